"""Refining predicted surfels against their posed views (include/lara_splatadam.h, csrc/splatadam.hip): a few dozen optimisation steps
on a ``splatio.SurfelCloud`` -- ``Renderer.render_views`` (one autograd node), ``loss.lara_loss``, ``backward``, and the parameter
update of the Gaussian-splatting code bases as ONE kernel launch over the five tensors.  Opt-in like every module here, imported by
nothing on the default routes; ``splatio``, ``splatxform``, the renderer and the loss are untouched.

  * ``plan``         the float64 row of one step: the betas, the bias corrections of step t, eps, six learning rates;
  * ``adam_step``    the functional form, on either device: five parameters, gradients and moment pairs under one plan;
  * ``SurfelAdam``   the optimiser object: leaf tensors, moments, the step count, ``step`` / ``zero_grad`` / ``cloud`` / ``state``;
  * ``refine``       the loop: render, loss, backward, the rasteriser's own radii as the visibility mask, step.  No host read inside.

The update is ``torch.optim.Adam``'s formula in double on the fp32 words, rounded once at each store (include/lara_splatadam.h has the
operation order), with three gates ``torch.optim.Adam`` cannot express in one pass:
  visible     surfels no view saw in a step keep their parameters AND their moments, bit for bit (3DGS's "sparse Adam" [RECALLED:
              neither code base is in the build image]); ``visible=None`` is dense mode, ``torch.optim.Adam``'s semantics;
  non-finite  a gradient word that is inf or NaN skips its element and is counted, so a cloud stays finite;
  zero_grads  the gradients are zeroed by the launch that consumed them.
The six learning rates are: centres, SH coefficient 0, SH coefficients >= 1, opacity, scales, rotations; the defaults are the 2DGS
training arguments as recalled [RECALLED: position_lr_init 1.6e-4, feature_lr 2.5e-3 (a twentieth of it for the higher bands),
opacity_lr 0.05, scaling_lr 5e-3, rotation_lr 1e-3; nothing pins them].

Tensors on the GPU go through the kernel.  Tensors on the host go through ``lara_splatadam_step_host``, the same per-word function
compiled for the CPU (csrc/splatadam_ops.h): the reference the kernel is held to bit for bit, not a fast path.

The trap: the kernel writes through ``data_ptr()``, which does not advance torch's version counter, and ``Renderer._activated``
reuses its cached sigmoid / exp / normalize while address and version are unchanged.  ``SurfelAdam.step`` bumps the version of every
parameter; a caller of ``adam_step`` on tensors a renderer has seen calls ``bump_version`` (or ``invalidate_activations``) itself.

Densification (clone, split, prune, opacity reset) is ``lara_amd.splatdensify``: ``refine(..., densify=DensifySchedule(...))``,
``SurfelAdam.densify`` and ``SurfelAdam.reset_opacity`` import it when they are used, nothing else here does.

Out of scope: per-surfel step counts (one ``t`` for the cloud: a surfel first seen at
step 50 is bias-corrected as at step 50), weight decay, learning-rate schedules (beyond an ``lrs`` the caller may change between
steps), gradients through ``splatxform``, camera refinement.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import splatio
from . import _native
from ._native import host_array

PLAN = 13                                # include/lara_splatadam.h
SPAN = 256
FIELDS = splatio.SurfelCloud.FIELDS
LR_KEYS = ("centers", "sh0", "sh_rest", "opacity", "scales", "rotations")
DEFAULT_LRS = {"centers": 1.6e-4, "sh0": 2.5e-3, "sh_rest": 2.5e-3 / 20.0, "opacity": 0.05, "scales": 5e-3, "rotations": 1e-3}
_WHO = "lara_amd.splatrefine"


# ---------------------------------------------------------------------------------------------------------- the plan

def _rates(lrs):
    if lrs is None:
        lrs = DEFAULT_LRS
    if isinstance(lrs, dict):
        unknown = set(lrs) - set(LR_KEYS)
        if unknown:
            raise ValueError(f"{_WHO}: unknown learning rates {sorted(unknown)}; the six are {LR_KEYS}")
        return [float(lrs.get(k, DEFAULT_LRS[k])) for k in LR_KEYS]
    lrs = [float(v) for v in lrs]
    if len(lrs) != len(LR_KEYS):
        raise ValueError(f"{_WHO}: six learning rates {LR_KEYS}, got {len(lrs)}")
    return lrs


def plan(step, lrs=None, betas=(0.9, 0.999), eps=1e-15):
    """The plan of step ``step`` (1-based, as ``torch.optim.Adam`` counts) as 13 float64 (numpy): [0] b1, [1] 1 - b1, [2] b2,
    [3] 1 - b2, [4] bc1 = 1 - b1^t, [5] sqrt(1 - b2^t), [6] eps, [7:13] the learning rates of centres, SH coefficient 0, SH
    coefficients >= 1, opacity, scales, rotations.  ``lrs``: a dict over ``LR_KEYS`` (missing keys take the default) or six numbers;
    the defaults are the 2DGS training arguments as recalled [RECALLED]: 1.6e-4, 2.5e-3, 2.5e-3 / 20, 0.05, 5e-3, 1e-3.  Every value
    is computed in float64 on the host; the kernel runs no pow."""
    t = int(step)
    b1, b2 = float(betas[0]), float(betas[1])
    if t < 1 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or not float(eps) >= 0.0:
        raise ValueError(f"{_WHO}: a plan needs step >= 1, betas in [0, 1) and eps >= 0, got {step!r}, {betas!r}, {eps!r}")
    row = np.empty(PLAN, np.float64)
    row[0:7] = b1, 1.0 - b1, b2, 1.0 - b2, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), float(eps)
    row[7:13] = _rates(lrs)
    return row


# ---------------------------------------------------------------------------------------------------------- the step

def bump_version(tensors):
    """Advance torch's version counter of every tensor: what a write through ``data_ptr()`` does not do."""
    inc = getattr(torch.autograd.graph, "increment_version", None)
    for t in tensors:
        if inc is not None:
            inc(t)
        else:
            with torch.no_grad():
                t[:0].zero_()                # (a zero-length in-place operation on a view: the base's counter moves, no word does)


@torch.no_grad()
def adam_step(params, grads, exp_avg, exp_avg_sq, plan, visible=None, zero_grads=False, counters=None):
    """One step in place: ``params``, ``grads``, ``exp_avg``, ``exp_avg_sq`` are each the five tensors of a cloud (centers [P,3], shs
    [P,n,3], opacity [P,1], scales [P,2], rotations [P,4]; fp32, contiguous, one device), ``plan`` the 13 doubles of ``plan()``.
    ``visible``: None (dense) or uint8 / bool [P] -- rows with 0 keep parameter and moment words.  ``zero_grads``: +0.0 over every
    gradient word.  ``counters``: an int64 tensor of one element on the same device, to which the number of elements skipped for a
    non-finite gradient is ADDED (None: a fresh zero).  Returns ``counters``.  One kernel launch, no host read, on the GPU; the host
    entry for host tensors.  The version counters are not advanced (``bump_version``).  ValueError: a non-contiguous tensor, a wrong
    dtype, mixed devices, a gradient or moment whose shape differs from its field's."""
    params = splatio.check_fields(_WHO, "params", params)
    grads, exp_avg, exp_avg_sq = (splatio.check_fields(_WHO, w, ts, like=params) for w, ts in (("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)))
    dev, P, n = params[0].device, params[0].shape[0], params[1].shape[1]
    row = np.asarray(plan, np.float64)
    if row.shape != (PLAN,):
        raise ValueError(f"{_WHO}: a plan is {PLAN} doubles (splatrefine.plan), got {row.shape}")
    if visible is not None:
        if not isinstance(visible, torch.Tensor) or tuple(visible.shape) != (P,) or visible.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{_WHO}: visible is a uint8 or bool tensor [{P}]")
        if visible.device != dev or not visible.is_contiguous():
            raise ValueError(f"{_WHO}: visible must be contiguous on {dev}, got {visible.device}")
        if visible.dtype == torch.bool:
            visible = visible.view(torch.uint8)                                # (a bool tensor's bytes are 0 and 1)
    if counters is None:
        counters = torch.zeros(1, dtype=torch.int64, device=dev)
    elif (not isinstance(counters, torch.Tensor) or counters.dtype != torch.int64 or counters.numel() != 1 or counters.device != dev
          or not counters.is_contiguous()):
        raise ValueError(f"{_WHO}: counters is one int64 on {dev}")
    if P == 0:                               # (an empty tensor has no address to hand over; nothing is launched)
        return counters
    _native.call_on("lara_splatadam_step", dev, host_array("d", row.tolist()), splatio.SH_COEFFS[n], P,
                    *params, *grads, *exp_avg, *exp_avg_sq, visible, 1 if zero_grads else 0, counters)
    return counters


# ---------------------------------------------------------------------------------------------------------- the optimiser

class SurfelAdam:
    """The optimiser of one cloud.  It owns contiguous clones of the cloud's five tensors as leaf tensors that require grad
    (``params()``: what ``Renderer.render_views`` takes), their two moments and the step count.  ``sparse``: ``step(visible)`` gates
    rows by ``visible``; with ``sparse=False`` every step is dense and ``visible`` is ignored.  ``lrs`` (a dict over ``LR_KEYS``)
    may be changed between steps."""

    def __init__(self, cloud, lrs=None, betas=(0.9, 0.999), eps=1e-15, sparse=True):
        self.lrs = dict(zip(LR_KEYS, _rates(lrs)))
        self.betas, self.eps, self.sparse = (float(betas[0]), float(betas[1])), float(eps), bool(sparse)
        plan(1, self.lrs, self.betas, self.eps)                                  # (refuses bad betas / eps now, not at the first step)
        self._params = [t.detach().clone(memory_format=torch.contiguous_format).requires_grad_(True) for t in cloud.render_args()]
        self.exp_avg = [torch.zeros_like(p) for p in self._params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self._params]
        self.steps = 0
        self.skipped = torch.zeros(1, dtype=torch.int64, device=cloud.device)     # elements skipped for a non-finite gradient, so far

    def params(self):
        """(centers, shs, opacity, scales, rotations): the leaf tensors, in ``render_views``' order."""
        return tuple(self._params)

    def step(self, visible=None, zero_grads=False):
        """One update from the parameters' ``.grad`` (``backward`` has run).  ``visible``: bool or uint8 [P], used when ``sparse``.
        Advances every parameter's version counter, so that a renderer's cached activations are not reused."""
        grads = []
        for name, p in zip(FIELDS, self._params):
            if p.grad is None:
                raise RuntimeError(f"{_WHO}: {name} has no gradient; run backward before step")
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            grads.append(p.grad)
        self.steps += 1
        adam_step([p.detach() for p in self._params], grads, self.exp_avg, self.exp_avg_sq,
                  plan(self.steps, self.lrs, self.betas, self.eps), visible if self.sparse else None, zero_grads, self.skipped)
        bump_version(self._params)

    def zero_grad(self):
        """+0.0 over the gradients that exist (they stay allocated); ``step(zero_grads=True)`` does it in the step's launch."""
        for p in self._params:
            if p.grad is not None:
                p.grad.zero_()

    def cloud(self):
        """A detached ``SurfelCloud`` holding a copy of the current values."""
        return splatio.SurfelCloud(*(p.detach().clone() for p in self._params))

    def state(self):
        """What ``load_state`` takes: the step count, copies of the parameters and moments, the settings."""
        return {"steps": self.steps, "params": [p.detach().clone() for p in self._params], "exp_avg": [t.clone() for t in self.exp_avg],
                "exp_avg_sq": [t.clone() for t in self.exp_avg_sq], "skipped": self.skipped.clone(), "lrs": dict(self.lrs),
                "betas": self.betas, "eps": self.eps, "sparse": self.sparse}

    @torch.no_grad()
    def load_state(self, state):
        """Take over a ``state()``: the words are copied into this optimiser's own tensors (same shapes), the versions advance."""
        dev = self._params[0].device
        for mine, key in ((self._params, "params"), (self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
            theirs = splatio.check_fields(_WHO, f"state[{key!r}]", [t.to(dev) for t in state[key]], like=mine)
            for a, b in zip(mine, theirs):
                a.copy_(b)
        self.skipped.copy_(state["skipped"].to(dev))
        self.steps = int(state["steps"])
        self.lrs, self.betas, self.eps, self.sparse = dict(state["lrs"]), tuple(state["betas"]), float(state["eps"]), bool(state["sparse"])

    def densify(self, stats, plan, noise=None, seed=0, max_surfels=None):
        """One round of ``splatdensify.densify`` on this optimiser's cloud: the leaf tensors and the moments are REPLACED by the new
        ones (another row count; kept rows carry their moments, clones and split children start from zero), ``steps`` stays, the
        gradients are gone.  Returns the round's report.  ``stats`` no longer fits afterwards: ``stats.reset(report["P_out"])``."""
        from . import splatdensify
        p, m, v, report = splatdensify.densify([t.detach() for t in self._params], self.exp_avg, self.exp_avg_sq, stats, plan, noise=noise,
                                               seed=seed, max_surfels=max_surfels)
        self._params = [t.requires_grad_(True) for t in p]
        self.exp_avg, self.exp_avg_sq = m, v
        bump_version(self._params)
        return report

    def reset_opacity(self, ceiling=0.01):
        """``splatdensify.reset_opacity`` on this optimiser's opacity and its two moments, in place."""
        from . import splatdensify
        splatdensify.reset_opacity(self._params, self.exp_avg, self.exp_avg_sq, ceiling=ceiling)


# ---------------------------------------------------------------------------------------------------------- the loop

MS_SSIM_MIN = 160                        # the five-scale pyramid with an 11-tap window needs more than this on both sides


def _default_loss(batch, output, it):
    from . import loss
    H, VW = output["image"].shape[1:3]
    return loss.lara_loss(batch, output, it=it, ms_ssim=H > MS_SSIM_MIN and VW > MS_SSIM_MIN)


def refine(cloud, cams, rays, targets, *, steps, lrs=None, sparse=True, bg_colors=None, renderer=None, regularise_after=None, loss_fn=None,
           views_per_step=None, seed=0, callback=None, densify=None):
    """``steps`` optimisation steps of ``cloud`` against ``targets`` [V,H,W,3] (fp32 in 0..1, on the cloud's device) seen from
    ``cams`` (``cameras.make_cameras``) with ``rays`` [V,H,W,6] (``batch.build_rays``).  Returns (the refined ``SurfelCloud``,
    history).  Per step: ``render_views(..., concat=True, raster_out=...)``, the loss, ``backward``, ``visible = (radii > 0).any(0)``
    from the rasteriser's own radii when ``sparse``, ``SurfelAdam.step`` (which also zeroes the gradients).  No host read in the loop.

    ``loss_fn(batch, output, it) -> (loss, stats with "mse")``: the default is ``loss.lara_loss`` on the concatenated maps with a
    leading batch axis -- the reference's own weighting (lightning/loss.py:35-60) -- with ``it`` chosen so that the distortion and
    normal terms switch on after ``regularise_after`` steps (None: never), and the MS-SSIM term only where both H and V W exceed 160
    (below, the five-scale pyramid is undefined).  ``views_per_step``: that many views drawn per step (a host generator seeded with
    ``seed``; None: all).  ``bg_colors``: [V,3] per-view backgrounds.  ``callback(step, optimiser, loss)`` after every step.
    ``history``: ``loss`` and ``mse`` [steps] as device tensors (read them once, at the end), ``skipped`` (the non-finite counter),
    ``steps``, and ``optimiser`` (the ``SurfelAdam``, for its ``state()``).

    ``densify``: a ``splatdensify.DensifySchedule`` (None: the loop above, exactly).  With one, every render gets a ``means2D`` that
    requires grad, ``splatdensify.DensifyStats.accumulate`` runs after each backward on its gradient and the radii (per render call,
    not per view: ``views_per_step=1`` gives 3DGS's statistic), and after the update of the steps the schedule names the cloud is
    densified (``SurfelAdam.densify``) -- the statistics start again at the new surfel count -- or its opacity reset.
    ``history["densify"]`` gets one entry per round: ``step`` (1-based), ``counts`` (kept, cloned, split parents, pruned, P_out as an
    int64 device tensor), ``row_source`` and ``capped``.  The one host read a round needs is the allocation's."""
    from .renderer import Renderer
    dev = cloud.device
    _native.require_device(dev)
    V = len(cams)
    rays = rays if torch.is_tensor(rays) else torch.stack(list(rays))
    if not torch.is_tensor(targets) or targets.dim() != 4 or targets.shape[0] != V or targets.shape[-1] != 3 or rays.shape[:3] != targets.shape[:3]:
        raise ValueError(f"{_WHO}: targets is [V,H,W,3] for the {V} cameras and rays [V,H,W,6], got {tuple(targets.shape)} and {tuple(rays.shape)}")
    if targets.device != dev or rays.device != dev:
        raise ValueError(f"{_WHO}: targets and rays lie on {targets.device} and {rays.device}, the cloud on {dev}")
    targets = targets.float().contiguous()
    n_step = V if views_per_step is None else int(views_per_step)
    if not 1 <= n_step <= V or int(steps) < 0:
        raise ValueError(f"{_WHO}: views_per_step in 1..{V} and steps >= 0, got {views_per_step!r} and {steps!r}")
    renderer = renderer if renderer is not None else Renderer(sh_degree=cloud.sh_degree, white_background=True)
    loss_fn = loss_fn if loss_fn is not None else _default_loss
    opt = SurfelAdam(cloud, lrs=lrs, sparse=sparse)
    draw = torch.Generator().manual_seed(int(seed))
    history = {"loss": torch.zeros(int(steps), dtype=torch.float32, device=dev), "mse": torch.zeros(int(steps), dtype=torch.float32, device=dev),
               "skipped": opt.skipped, "steps": int(steps), "optimiser": opt}
    stats = means2D = None
    if densify is not None:
        from . import splatdensify
        if not isinstance(densify, splatdensify.DensifySchedule):
            raise ValueError(f"{_WHO}: densify is a splatdensify.DensifySchedule, got {type(densify).__name__}")
        stats = splatdensify.DensifyStats(cloud.n_surfels, dev)
        history["densify"] = []
    for k in range(int(steps)):
        if stats is not None:
            means2D = torch.zeros_like(opt.params()[0], requires_grad=True)
        if n_step == V:
            v_cams, v_rays, v_tar, v_bg = list(cams), rays, targets, bg_colors
        else:
            idx = torch.randperm(V, generator=draw)[:n_step].tolist()           # (a host generator: no device is asked)
            v_cams, v_rays, v_tar = [cams[i] for i in idx], rays[idx], targets[idx]
            v_bg = None if bg_colors is None else bg_colors[idx]
        raster_out = []
        out = renderer.render_views(v_cams, v_rays, *opt.params(), dev, bg_colors=v_bg, concat=True, raster_out=raster_out, means2D=means2D)
        output = {name: m[None] for name, m in out.items()}
        it = 10000 if regularise_after is not None and k >= int(regularise_after) else 0      # (loss.py:47 switches at it > 1000)
        loss, terms = loss_fn({"tar_rgb": v_tar[None]}, output, it)
        loss.backward()
        visible = (raster_out[0][1] > 0).any(0) if sparse else None
        if stats is not None:
            stats.accumulate(means2D.grad, raster_out[0][1])
        opt.step(visible, zero_grads=True)
        history["loss"][k] = loss.detach()
        history["mse"][k] = terms["mse"]
        if stats is not None and densify.fires(k + 1):
            report = opt.densify(stats, densify.plan(), seed=int(densify.seed) + k, max_surfels=densify.max_surfels)
            if report["P_out"] == 0:
                raise RuntimeError(f"{_WHO}: the densification round of step {k + 1} pruned every surfel")
            stats.reset(report["P_out"])
            history["densify"].append({"step": k + 1, "counts": report["counts"], "row_source": report["row_source"], "capped": report["capped"]})
        if stats is not None and densify.resets(k + 1):
            opt.reset_opacity()
        if callback is not None:
            callback(k, opt, loss.detach())
    return opt.cloud(), history
