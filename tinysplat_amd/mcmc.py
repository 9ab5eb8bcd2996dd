"""Budgeted densification: 3DGS-MCMC relocation, growth to a cap and position noise on the GPU.

Not in the reference, whose densifier stops growing at a million Gaussians wherever the gradient threshold took it
(``densify.MAX_GAUSSIANS``).  Here the user names the count: dead Gaussians (``sigmoid(opacity) <= min_opacity``) are
moved onto live ones drawn in proportion to opacity, with opacity and scale corrected so that the image is unchanged to
first order (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", NeurIPS 2024); the set grows by 5 %
per refinement up to ``cap_max``; a covariance-shaped noise on the positions of near-transparent Gaussians keeps them
exploring; two small regularisers, ``mean(sigmoid(opacities))`` and ``mean(exp(scales))``, make Gaussians die.  Once the
cap is reached N never changes and nothing is reallocated.

``McmcDensifier`` has the hooks ``training.TrainStep`` calls on a densifier, so ``TrainStep(...)(..., densifier=)`` and
``fit(..., densifier=)`` take it as they take ``densify.Densifier``.  The plain ops (``sample_rows``, ``relocation``,
``inject_noise``, ``mcmc_normals``, ``mean_opacity``, ``mean_scale``) are the C entries of csrc/mcmc.hip one by one.
There is no CPU path: tensors must be on the GPU.  The sharded trainer does not take this densifier.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._rows import compact, fields_of, hold, install, plan, rebuild, tables
from .ops import _call, _f32c, _need_hip, _ptr, _stream

N_MAX = 51                      # TS_MCMC_N_MAX
_MEAN_SIGMOID, _MEAN_EXP = 0, 1


@dataclass
class McmcConfig:
    """gsplat's ``MCMCStrategy`` defaults."""
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    min_opacity: float = 0.005
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    refine_start: int = 500
    refine_stop: int = 25_000
    refine_every: int = 100
    grow_percent: int = 105          # a refinement grows N to min(cap_max, N * grow_percent // 100)

    def fires(self, step: int) -> bool:
        """True on the steps a refinement runs: ``refine_start < step < refine_stop`` and a multiple of ``refine_every``."""
        return self.refine_start < step < self.refine_stop and step % self.refine_every == 0


class ExponentialLr:
    """3DGS's log-linear decay of the means' learning rate, ``exp((1 - t) ln lr0 + t ln lr1)`` with ``t = step /
    max_steps`` clamped to [0, 1] (the reference's ``update_learning_rate`` TODO, model_gaussian.py:122-124).  A
    ``lr_schedule`` of ``training.fit``: ``step -> {"means": lr}``."""

    def __init__(self, initial: float, final: float, max_steps: int, name: str = "means"):
        if not (initial > 0 and final > 0 and max_steps >= 1):
            raise ValueError("ExponentialLr needs positive rates and max_steps >= 1")
        self.initial, self.final, self.max_steps, self.name = float(initial), float(final), int(max_steps), name

    def __call__(self, step: int) -> Dict[str, float]:
        t = min(max(step / self.max_steps, 0.0), 1.0)
        return {self.name: math.exp((1.0 - t) * math.log(self.initial) + t * math.log(self.final))}


# ------------------------------------------------------------------------------------------------ plain ops
@torch.no_grad()
def sample_rows(weights: Tensor, u: Tensor) -> Tuple[Tensor, Tensor]:
    """``u`` (float32 [M] in [0, 1)) -> (picks int32 [M], counts int32 [N]) over ``weights`` (float64 [N], >= 0): draw j
    picks the first row whose inclusive prefix (double, the fixed order of ``sample_points``'s scan) exceeds ``u[j]``
    times the total; a row of weight 0 is never picked.  ``counts`` is how often each row was picked."""
    dev = _need_hip(weights, u)
    if weights.dtype != torch.float64 or weights.dim() != 1 or weights.shape[0] < 1:
        raise ValueError("weights must be float64 [N], N >= 1")
    weights, u = weights.contiguous(), _f32c(u)
    if u.dim() != 1 or u.shape[0] < 1:
        raise ValueError("u must be float32 [M], M >= 1")
    n, m = weights.shape[0], u.shape[0]
    lib = _lib.load()
    ws = torch.empty((int(lib.ts_mcmc_sample_ws_bytes(n)),), dtype=torch.uint8, device=dev)
    picks = torch.empty((m,), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_mcmc_sample_rows", lib.ts_mcmc_sample_rows, n, m, _ptr(weights), _ptr(u), _ptr(picks), _ptr(counts),
              _ptr(ws), _stream(dev))
    return picks, counts


def _rewrite(opacities: Tensor, scales: Tensor, counts: Tensor, min_opacity: float, moments=None) -> None:
    dev = opacities.device
    n = opacities.shape[0]
    k = 0 if moments is None else len(moments[0])
    args = (None, None, None) if k == 0 else tables(*moments)          # exp_avg, exp_avg_sq, widths
    with torch.cuda.device(dev):
        _call("ts_mcmc_rewrite", _lib.load().ts_mcmc_rewrite, n, _ptr(counts), float(min_opacity), _ptr(opacities),
              _ptr(scales), k, *args, _stream(dev))


@torch.no_grad()
def relocation(opacities: Tensor, scales: Tensor, counts: Tensor, config: Optional[McmcConfig] = None):
    """-> (opacities, scales) with every row of ``counts[i] > 0`` (int32 [N]) rewritten as a source that ``counts[i]``
    draws picked: ``M = min(counts[i] + 1, 51)``, ``o' = 1 - (1 - o)^(1/M)``, the logit of ``clamp(o', min_opacity,
    1 - 2^-23)`` and log-scales grown by ``log(o / D)``.  Other rows are copied.  The inputs are not modified."""
    dev = _need_hip(opacities, scales, counts)
    cfg = config or McmcConfig()
    n = opacities.shape[0]
    if opacities.numel() != n or scales.shape != (n, 3) or counts.shape != (n,) or counts.dtype != torch.int32 or n < 1:
        raise ValueError("opacities [N,1], scales [N,3] float32 and counts [N] int32, N >= 1")
    o, s = _f32c(opacities.detach()).clone(), _f32c(scales.detach()).clone()
    _rewrite(o, s, counts.contiguous(), cfg.min_opacity)
    return o, s


@torch.no_grad()
def mcmc_normals(n: int, seed: int, step: int, device) -> Tensor:
    """float32 [n,3]: exactly the unit normals ``inject_noise(z=None, seed, step)`` draws inside its kernel."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("tinysplat_amd ops run only on a HIP (cuda) device. There is deliberately no CPU fallback.")
    if n < 1:
        raise ValueError("n must be positive")
    out = torch.empty((int(n), 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(out.device):
        _call("ts_mcmc_normals", _lib.load().ts_mcmc_normals, int(n), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF,
              _ptr(out), _stream(out.device))
    return out


@torch.no_grad()
def inject_noise(model, scale: float, z: Optional[Tensor] = None, seed: int = 0, step: int = 0) -> None:
    """``means += scale * g(1 - o) * (Sigma z)`` in place, ``o = sigmoid(opacities)``, ``g(x) = 1 / (1 + exp(-100 (x -
    0.995)))``, ``Sigma = R diag(exp(2 scales)) R^T``.  ``z``: float32 [N,3] unit normals; None: drawn in the kernel from
    Philox4x32-10 keyed by ``seed`` with counter (row, step).  Rows of high opacity (g exactly 0) keep their bits."""
    means, scales, quats, opac = model.means, model.scales, model.quats, model.opacities
    dev = _need_hip(means, scales, quats, opac)
    n = means.shape[0]
    if n < 1:
        return
    for t in (means, scales, quats, opac):
        if not t.is_contiguous() or t.dtype != torch.float32 or t.shape[0] != n:
            raise ValueError(f"the noise needs contiguous float32 tensors of {n} rows")
    if z is not None:
        z = _f32c(z)
        if z.shape != (n, 3) or z.device != dev:
            raise ValueError(f"z must be [{n}, 3] on {dev}")
    with torch.cuda.device(dev):
        _call("ts_mcmc_noise", _lib.load().ts_mcmc_noise, n, _ptr(means), _ptr(scales), _ptr(quats), _ptr(opac),
              float(scale), _ptr(z), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, _stream(dev))


class _Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        dev = _need_hip(x)
        xc = _f32c(x)
        count = xc.numel()
        if count < 1:
            raise ValueError("the mean needs at least one element")
        lib = _lib.load()
        ws = torch.empty((int(lib.ts_mcmc_mean_ws_bytes(count)),), dtype=torch.uint8, device=dev)
        value = torch.empty((), dtype=torch.float32, device=dev)
        grad = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            _call("ts_mcmc_mean", lib.ts_mcmc_mean, kind, count, _ptr(xc), _ptr(value), _ptr(grad), _ptr(ws), _stream(dev))
        ctx.save_for_backward(grad)
        ctx.shape = x.shape
        return value

    @staticmethod
    def backward(ctx, v):
        (grad,) = ctx.saved_tensors
        return (None if grad is None else (grad * v).view(ctx.shape)), None


def mean_opacity(opacities: Tensor) -> Tensor:
    """``mean(sigmoid(opacities))`` as a 0-dim tensor, differentiable; the sum is taken in double in a fixed order."""
    return _Mean.apply(opacities, _MEAN_SIGMOID)


def mean_scale(scales: Tensor) -> Tensor:
    """``mean(exp(scales))`` over every element, as a 0-dim tensor, differentiable; double sum in a fixed order."""
    return _Mean.apply(scales, _MEAN_EXP)


# ------------------------------------------------------------------------------------------------ the densifier
class McmcDensifier:
    """The budgeted strategy behind ``TrainStep``'s densifier hooks.  ``generator`` draws the rows of a refinement (torch's
    default generator of the device otherwise); ``seed`` keys the in-kernel normals of the noise, whose counter is the
    step.  ``last_counts = (dead, relocated, added, N)`` of the last refinement."""

    def __init__(self, model, config: Optional[McmcConfig] = None, generator: Optional[torch.Generator] = None,
                 seed: int = 0):
        self.model = model
        self.cfg = config or McmcConfig()
        self.generator, self.seed = generator, int(seed)
        self.last_counts = None
        self.last_dead = 0                           # dead rows the last relocation found
        self.last_picks = self.last_pick_counts = self.last_dead_rows = None     # the last draws (for tests)
        hold(model, "McmcDensifier")

    # ---- the hooks
    def update_grad_accum(self, step: int, extras) -> None:
        """Nothing: this strategy does not look at gradients."""

    def loss_terms(self, model, step: int) -> Dict[str, tuple]:
        c, out = self.cfg, {}
        if c.opacity_reg != 0:
            out["opacity_reg"] = (float(c.opacity_reg), mean_opacity(model.opacities))
        if c.scale_reg != 0:
            out["scale_reg"] = (float(c.scale_reg), mean_scale(model.scales))
        return out

    @torch.no_grad()
    def densify_and_prune(self, step: int, optim, extras=None, u: Optional[Tensor] = None) -> bool:
        """On the schedule's steps: relocate, then add.  Then, on every step, the noise at ``optim.lrs['means'] *
        noise_lr``.  ``u`` (tests): float32 uniforms, the first ``dead`` of them for the relocation and the following
        ``n_new`` for the growth.  Returns whether the parameter tensors were replaced."""
        replaced = self.refine(optim, u) if self.cfg.fires(step) else False
        if self.cfg.noise_lr != 0:
            inject_noise(self.model, float(optim.lrs["means"]) * float(self.cfg.noise_lr), None, self.seed, step)
        return replaced

    @torch.no_grad()
    def update_state(self, optim, mask: Tensor, _tensors=None) -> None:
        """``Densifier.update_state`` without an accumulator: drop the rows where ``mask`` is True, append the caller's."""
        compact(self.model, optim, mask, _tensors)

    # ---- a refinement
    def _uniforms(self, m: int, u: Optional[Tensor], used: int, dev) -> Tensor:
        if u is None:
            if self.generator is None:
                return torch.rand((m,), dtype=torch.float32, device=dev)
            return torch.rand((m,), dtype=torch.float32, generator=self.generator, device=self.generator.device).to(dev)
        if u.dim() != 1 or u.shape[0] < used + m:
            raise ValueError(f"u must hold at least {used + m} uniforms")
        return _f32c(u[used:used + m].to(dev))

    @torch.no_grad()
    def relocate(self, optim, u: Optional[Tensor] = None, _used: int = 0) -> int:
        """Moves every dead row onto a live row drawn in proportion to opacity -> the number of rows moved (0 when no
        row or every row is dead).  ``self.last_dead`` is the number of dead rows found."""
        old, live, n, dev = fields_of(self.model)
        lib = _lib.load()
        with torch.cuda.device(dev):
            w = torch.empty((n,), dtype=torch.float64, device=dev)
            flags = torch.empty((n,), dtype=torch.uint8, device=dev)
            _call("ts_mcmc_weights", lib.ts_mcmc_weights, n, _ptr(old["opacities"].detach()), float(self.cfg.min_opacity),
                  1, _ptr(w), _ptr(flags), _stream(dev))
        (dead, _, _, _), dead_rows = plan(flags, n, dev)       # the dead rows, ascending; the host read sizes the draws
        self.last_dead = dead
        if dead == 0 or dead == n:
            return 0
        picks, counts = sample_rows(w, self._uniforms(dead, u, _used, dev))
        moments = [optim.exp_avg[f] for f in live], [optim.exp_avg_sq[f] for f in live]
        _rewrite(old["opacities"].detach(), old["scales"].detach(), counts, self.cfg.min_opacity, moments)
        with torch.cuda.device(dev):
            _call("ts_mcmc_copy_rows", lib.ts_mcmc_copy_rows, n, dead, _ptr(dead_rows), _ptr(picks), len(live),
                  *tables([old[f] for f in live], *moments), _stream(dev))
        self.last_picks, self.last_pick_counts, self.last_dead_rows = picks, counts, dead_rows[:dead]
        return dead

    @torch.no_grad()
    def add(self, optim, u: Optional[Tensor] = None, _used: int = 0) -> int:
        """Grows the set to ``min(cap_max, N * 105 // 100)`` rows: the new rows are copies of rows drawn over ALL rows in
        proportion to opacity (rewritten first), appended in draw order -> their number.  0: nothing is reallocated."""
        old, live, n, dev = fields_of(self.model)
        n_new = min(int(self.cfg.cap_max), n * int(self.cfg.grow_percent) // 100) - n
        if n_new <= 0:
            return 0
        lib = _lib.load()
        with torch.cuda.device(dev):
            w = torch.empty((n,), dtype=torch.float64, device=dev)
            _call("ts_mcmc_weights", lib.ts_mcmc_weights, n, _ptr(old["opacities"].detach()), float(self.cfg.min_opacity),
                  0, _ptr(w), None, _stream(dev))
        picks, counts = sample_rows(w, self._uniforms(n_new, u, _used, dev))
        picks.clamp_(min=0)                            # (every opacity 0 or NaN: no row was drawn; the copies are row 0)
        _rewrite(old["opacities"].detach(), old["scales"].detach(), counts, self.cfg.min_opacity,
                 ([optim.exp_avg[f] for f in live], [optim.exp_avg_sq[f] for f in live]))
        src_of = torch.cat((torch.arange(n, dtype=torch.int32, device=dev), picks))
        install(self.model, optim, *rebuild(old, live, optim, src_of, n + n_new, n + n_new, n))   # new rows: zero moments
        self.last_picks, self.last_pick_counts = picks, counts
        return n_new

    @torch.no_grad()
    def refine(self, optim, u: Optional[Tensor] = None) -> bool:
        """One refinement: relocate, then add.  -> whether the parameter tensors were replaced."""
        moved = self.relocate(optim, u, 0)
        added = self.add(optim, u, self.last_dead if moved else 0)
        self.last_counts = (self.last_dead, moved, added, self.model.means.shape[0])
        return added > 0
