"""Surface regularisers of the training loop (scripts/train.py:71-91): the opacity entropy and the SuGaR density term.

``opacity_entropy`` is ``-mean(o log(o + 1e-10) + (1 - o) log(1 - o + 1e-10))`` with ``o = sigmoid(opacities)``,
value and gradient in one C-ABI call (csrc/surface.hip).  The SuGaR density regulariser (train.py:77-91,
model_gaussian.py:244-326) is ``sample_points`` (update steps: sample points on the Gaussians, their 16 nearest
means, the inverse list) and ``density_loss`` (every active step: ``mean |d - approx|`` over the visible points, value
and gradient from csrc/density.hip); DESIGN.md section 6e.  ``SurfaceConfig`` holds the reference's command-line
defaults (train.py:201-202, :234-241) and ``SurfaceRegularizer`` the schedules (train.py:33-40, :77-79, :103-105,
:152-159); ``training.TrainStep`` / ``training.fit`` take one with ``surface=``.  There is no CPU fallback: tensors
must be on the GPU.  The SDF variant (``--regularize-sdf``) is not implemented: the reference cannot run it.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib
from ._rows import compact, hold
from .ops import _call, _f32c, _need_hip, _ptr, _stream


class _OpacityEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities):
        dev = _need_hip(opacities)
        x = _f32c(opacities)
        n = x.numel()
        if n < 1:
            raise ValueError("opacity_entropy needs at least one opacity")
        lib = _lib.load()
        ws = torch.empty((int(lib.ts_opacity_entropy_ws_bytes(n)),), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        v = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            _call("ts_opacity_entropy", lib.ts_opacity_entropy, n, _ptr(x), _ptr(loss), _ptr(v), _ptr(ws), _stream(dev))
        ctx.save_for_backward(v)
        ctx.shape = opacities.shape
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        (v,) = ctx.saved_tensors
        return None if v is None else (v * v_loss).view(ctx.shape)     # out of place: retain_graph re-runs this


def opacity_entropy(opacities: Tensor) -> Tensor:
    """train.py:71-75: ``-mean(o log(o + 1e-10) + (1 - o) log(1 - o + 1e-10))``, ``o = sigmoid(opacities)``, over
    every element of the float32 logits (any shape; the model's are [N, 1]).  A 0-dim tensor, differentiable
    w.r.t. ``opacities`` (autograd's gradient of that expression, the ``+1e-10`` terms included)."""
    return _OpacityEntropy.apply(opacities)


DENSITY_K = 16                  # knn_points(..., K=16) (model_gaussian.py:259)
DENSITY_ZNEAR = 0.001           # approximate_density_function(znear=0.001) (:276)
_PROJECTIONS = {"reference": 0, "screen": 1}
_WEIGHTS = {"reference": 0, "area": 1}
_ROW = 11                       # gradient row: means xyz | scales xyz | quats wxyz | opacity
_FROZEN = 10                    # per sample: xi xyz | exp(scales) xyz | quats wxyz, at sampling time


def _density_params(model):
    return model.means, model.scales, model.quats, model.opacities


def _identity(model):
    return tuple((t.data_ptr(), tuple(t.shape)) for t in _density_params(model))


@dataclass
class DensitySamples:
    """One draw of ``sample_points``: what the reference keeps in ``model.points`` (with its autograd graph) and
    ``model.knn_idxs``.  ``points`` float32 [M,3]; ``rows`` int32 [M] (each point's source Gaussian); ``frozen``
    float32 [M,10] (xi, exp(scales), quats of the source at sampling time: the retained graph's saved values);
    ``knn`` int32 [M,16] (the nearest means, ascending in (distance, index)); ``inv_keys`` / ``inv_perm`` the inverse
    list, every (point, slot) pair and then every point's source, sorted stably by Gaussian row; ``source`` the
    identity of the parameter tensors it was built from."""
    points: Tensor
    rows: Tensor
    frozen: Tensor
    knn: Tensor
    inv_keys: Tensor
    inv_perm: Tensor
    source: tuple

    @property
    def normals(self) -> Tensor:
        return self.frozen[:, 0:3]

    def matches(self, model) -> bool:
        """True while ``model``'s means / scales / quats / opacities are the tensors sampled from (not replaced by a
        rebuild, a prune or ``spatial_sort_``)."""
        return self.source == _identity(model)


def _draw(shape, fn, generator, dev):
    if generator is None:
        return fn(shape, device=dev)
    return fn(shape, generator=generator, device=generator.device).to(dev)


@torch.no_grad()
def sample_points(model, num_samples: int, weights: str = "reference", generator: Optional[torch.Generator] = None,
                  rows: Optional[Tensor] = None, normals: Optional[Tensor] = None,
                  uniforms: Optional[Tensor] = None) -> DensitySamples:
    """model_gaussian.py:318-326 and the neighbour search of :257-261 (``update_neighbors=True``).

    A point is ``means[i] + R(quats[i] / |quats[i]|) (exp(scales[i]) * xi)`` with ``xi ~ N(0, I)``.  Row ``i`` is
    drawn with weight ``C_i = a_0 + ... + a_i`` (``weights="reference"``: the reference passes the cumulative sums to
    ``torch.multinomial``) or ``a_i`` (``"area"``), ``a_i = prod(exp(scales[i]))``; the draw is the inverse CDF of a
    uniform over prefix sums in double.  ``uniforms`` (float32 [M] in [0, 1)) and ``normals`` (float32 [M,3]) default
    to ``torch.rand`` / ``torch.randn`` with ``generator`` (on its own device); ``rows`` (int [M]) replaces the draw.
    The reference's ``multinomial`` stream cannot be reproduced: the same seed gives other rows.  Needs at least 16
    Gaussians (the reference's k-NN would fail)."""
    from .init import _knn
    means, scales, quats, _ = _density_params(model)
    dev = _need_hip(means, scales, quats)
    n, m = means.shape[0], int(num_samples)
    if n < DENSITY_K:
        raise ValueError(f"the density regulariser needs at least {DENSITY_K} Gaussians, got {n}")
    if m < 1:
        raise ValueError("num_samples must be positive")
    if weights not in _WEIGHTS:
        raise ValueError(f"weights must be one of {sorted(_WEIGHTS)}")
    if rows is not None:
        rows = rows.to(device=dev, dtype=torch.int32).contiguous()
        if rows.shape != (m,):
            raise ValueError(f"rows must be [{m}]")
        if bool(((rows < 0) | (rows >= n)).any()):
            raise ValueError(f"rows must lie in [0, {n})")
    elif uniforms is None:
        uniforms = _draw((m,), torch.rand, generator, dev)
    if uniforms is not None and rows is None:
        uniforms = _f32c(uniforms.to(dev))
        if uniforms.shape != (m,):
            raise ValueError(f"uniforms must be [{m}]")
    if normals is None:
        normals = _draw((m, 3), torch.randn, generator, dev)
    normals = _f32c(normals.to(dev))
    if normals.shape != (m, 3):
        raise ValueError(f"normals must be [{m}, 3]")
    ps = [_f32c(t.detach()) for t in (means, scales, quats)]
    lib = _lib.load()
    ws = torch.empty((int(lib.ts_density_sample_ws_bytes(n)),), dtype=torch.uint8, device=dev)
    out_rows = torch.empty((m,), dtype=torch.int32, device=dev)
    points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    frozen = torch.empty((m, _FROZEN), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_density_sample", lib.ts_density_sample, n, m, _WEIGHTS[weights], *(_ptr(t) for t in ps),
              _ptr(uniforms if rows is None else None), _ptr(rows), _ptr(normals), _ptr(out_rows), _ptr(points),
              _ptr(frozen), _ptr(ws), _stream(dev))
    _, knn, _ = _knn(points, ps[0], DENSITY_K, False)
    inv_keys, inv_perm = torch.sort(torch.cat((knn.view(-1), out_rows)), stable=True)
    return DensitySamples(points, out_rows, frozen, knn, inv_keys, inv_perm, _identity(model))


def _camera_host(camera):
    vp = torch.cat((torch.as_tensor(camera.view_matrix).reshape(-1), torch.as_tensor(camera.proj_matrix).reshape(-1)))
    return (ctypes.c_float * 32)(*vp.detach().to("cpu", torch.float32).tolist())


def _density_launch(tensors, samples: DensitySamples, depth: Tensor, camera, projection: str, parts: bool,
                    grads: bool, depth_grad: bool):
    if projection not in _PROJECTIONS:
        raise ValueError(f"projection must be one of {sorted(_PROJECTIONS)}")
    means, scales, quats, opacities = (_f32c(t.detach()) for t in tensors)
    depth = _f32c(depth.detach())
    dev = _need_hip(means, scales, quats, opacities, depth, samples.points)
    n, m = means.shape[0], samples.points.shape[0]
    if depth.dim() != 2:
        raise ValueError("depth must be [H, W]")
    if samples.knn.shape != (m, DENSITY_K) or samples.source[0][1][0] != n:
        raise ValueError("the samples were built for another model: sample again")
    h, w = depth.shape
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    out = torch.empty((3,), **f32)
    ws = torch.empty((int(lib.ts_density_loss_ws_bytes(m)),), dtype=torch.uint8, device=dev)
    pp = [torch.empty((m,), **f32) for _ in range(3)] + [torch.empty((m,), dtype=torch.uint8, device=dev)] \
        if parts else [None] * 4
    grows = torch.empty((m * (DENSITY_K + 1), _ROW), **f32) if grads else None
    tkeys = torch.empty((m * 4,), dtype=torch.int32, device=dev) if grads else None
    tvals = torch.empty((m * 4,), **f32) if grads else None
    g, vd = None, None
    with torch.cuda.device(dev):
        s = _stream(dev)
        _call("ts_density_loss", lib.ts_density_loss, n, m, _ptr(samples.points), _ptr(samples.rows),
              _ptr(samples.frozen), _ptr(samples.knn), _ptr(means), _ptr(scales), _ptr(quats), _ptr(opacities), h, w,
              _ptr(depth), _camera_host(camera), _PROJECTIONS[projection], DENSITY_ZNEAR, _ptr(out),
              *(_ptr(t) for t in pp), _ptr(grows), _ptr(tkeys), _ptr(tvals), _ptr(ws), s)
        if grads:
            e = m * (DENSITY_K + 1)
            g = torch.empty((n, _ROW), **f32)
            sws = torch.empty((int(lib.ts_segment_sum_ws_bytes(e, _ROW)),), dtype=torch.uint8, device=dev)
            _call("ts_segment_sum", lib.ts_segment_sum, e, _ROW, n, _ptr(samples.inv_keys), _ptr(samples.inv_perm),
                  _ptr(grows), _ptr(out[1:2]), _ptr(g), _ptr(sws), s)
            if depth_grad:
                keys, perm = torch.sort(tkeys, stable=True)
                vd = torch.empty((h, w), **f32)
                dws = torch.empty((int(lib.ts_segment_sum_ws_bytes(m * 4, 1)),), dtype=torch.uint8, device=dev)
                _call("ts_segment_sum", lib.ts_segment_sum, m * 4, 1, h * w, _ptr(keys), _ptr(perm), _ptr(tvals),
                      _ptr(out[1:2]), _ptr(vd), _ptr(dws), s)
    return out, pp, g, vd


class _DensityLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, scales, quats, opacities, depth, samples, camera, projection):
        need = ctx.needs_input_grad
        out, _, g, vd = _density_launch((means, scales, quats, opacities), samples, depth, camera, projection,
                                        parts=False, grads=any(need[:5]), depth_grad=need[4])
        ctx.save_for_backward(g, vd)
        ctx.opacity_shape = opacities.shape
        return out[0]

    @staticmethod
    def backward(ctx, v_loss):
        g, vd = ctx.saved_tensors
        if g is None:
            return (None,) * 8
        # out of place: a retained graph may run this twice
        return (g[:, 0:3] * v_loss, g[:, 3:6] * v_loss, g[:, 6:10] * v_loss,
                (g[:, 10:11] * v_loss).view(ctx.opacity_shape), None if vd is None else vd * v_loss,
                None, None, None)


def density_loss(model, samples: DensitySamples, depth: Tensor, camera, projection: str = "reference") -> Tensor:
    """train.py:80-91 without the SDF branch: ``mean(|d[mask] - approx|)`` over the points of ``samples``, a 0-dim
    tensor differentiable w.r.t. ``model.means / scales / quats / opacities`` and ``depth`` (the rendered [H, W]
    plane).  ``d`` and ``beta`` read the current parameters; the points' own gradient goes to each source row
    through the values frozen at sampling time (the reference's retained graph).  ``projection``: ``"reference"``
    (no perspective divide, an unnormalised grid: nearly every point reads a border pixel) or ``"screen"`` (the
    depth at the pixel where the point projects).  NaN with zero gradients when no point is visible."""
    return _DensityLoss.apply(*_density_params(model), depth, samples, camera, projection)


@torch.no_grad()
def density_parts(model, samples: DensitySamples, depth: Tensor, camera, projection: str = "reference"):
    """Per point, forward only: ``(density, beta, approx, mask)`` - the density after the ``d > 1`` clamp, beta,
    ``exp(-0.5 (z_map - z)^2 / beta^2)`` (for every point; the loss reads it where ``mask`` is True) and the
    visibility mask (bool)."""
    _, (d, b, a, mk), _, _ = _density_launch(_density_params(model), samples, depth, camera, projection, parts=True,
                                             grads=False, depth_grad=False)
    return d, b, a, mk.bool()


@dataclass
class SurfaceConfig:
    """The reference's regulariser options (scripts/train.py:201-202, :234-241) with their command-line defaults:
    ``--regularize-opacity`` (off unless given), ``--lambda-opacity 0.2``, window steps [7000, 9000);
    ``--regularize-density`` (off), ``--lambda-density 0.2``, window [9000, 15000).  ``density_interval`` is
    ``--interval-densify`` (100), used only by the re-sample rule; ``density_samples`` the script's constant 100_000.
    ``density_projection`` / ``density_sample_weights``: ``"reference"`` keeps the reference's quirks;
    ``"screen"`` / ``"area"`` correct them.  ``density_prune_ungated``: also prune at ``regularize_density_start``
    when the density term is off, as the reference does (train.py:103-105 tests the start step only)."""
    regularize_opacity: bool = False
    lambda_opacity: float = 0.2
    regularize_opacity_start: int = 7000
    regularize_opacity_end: int = 9000
    regularize_density: bool = False
    lambda_density: float = 0.2
    regularize_density_start: int = 9000
    regularize_density_end: int = 15000
    density_interval: int = 100
    density_samples: int = 100_000
    density_projection: str = "reference"
    density_sample_weights: str = "reference"
    density_prune_ungated: bool = False

    def __post_init__(self):
        if self.density_projection not in _PROJECTIONS:
            raise ValueError(f"density_projection must be one of {sorted(_PROJECTIONS)}")
        if self.density_sample_weights not in _WEIGHTS:
            raise ValueError(f"density_sample_weights must be one of {sorted(_WEIGHTS)}")


class SurfaceRegularizer:
    """The schedules of train.py:33-40 (``Scheduler``: active for ``start <= step < end`` when enabled).
    ``terms(model, step)`` -> ``{name: (weight, differentiable scalar)}`` for the terms that need no render (the
    opacity entropy); ``frame_terms(model, step, camera, extras)`` the same for the density term, after the render;
    ``after_step(model, step, optimizer, densifier)`` the prune of train.py:103-105.  ``generator`` draws the
    samples."""

    def __init__(self, config: SurfaceConfig = None, generator: Optional[torch.Generator] = None):
        self.config = config if config is not None else SurfaceConfig()
        self.generator = generator
        self.samples: Optional[DensitySamples] = None

    def opacity_active(self, step: int) -> bool:
        c = self.config
        return bool(c.regularize_opacity) and c.regularize_opacity_start <= step < c.regularize_opacity_end

    def density_active(self, step: int) -> bool:
        c = self.config
        return bool(c.regularize_density) and c.regularize_density_start <= step < c.regularize_density_end

    def density_update(self, step: int) -> bool:
        """train.py:78: re-sample and re-search on the window's first step and whenever ``step % interval == 1``."""
        c = self.config
        return step == c.regularize_density_start or step % c.density_interval == 1

    def prune_due(self, step: int) -> bool:
        """train.py:103-105 prunes at ``regularize_density_start`` (the reference even with the term off:
        ``density_prune_ungated``)."""
        c = self.config
        return step == c.regularize_density_start and (bool(c.regularize_density) or bool(c.density_prune_ungated))

    def active(self, step: int) -> bool:
        return self.opacity_active(step) or self.density_active(step)

    def frame_terms(self, model, step: int, camera, extras) -> Dict[str, tuple]:
        """The density term at ``step`` on the rendered depth ``extras['depth']``: re-samples on the reference's
        update steps, and also (deviation) when the parameter tensors are not the ones sampled from, or when there
        are no samples yet (a resumed run) - the reference would index stale rows there."""
        if not self.density_active(step):
            return {}
        c = self.config
        if self.samples is None or self.density_update(step) or not self.samples.matches(model):
            self.samples = sample_points(model, c.density_samples, c.density_sample_weights, self.generator)
            hold(model, "SurfaceRegularizer")      # the neighbour indices are per-row state
        term = density_loss(model, self.samples, extras["depth"], camera, c.density_projection)
        return {"loss_density": (float(c.lambda_density), term)}

    @torch.no_grad()
    def after_step(self, model, step: int, optimizer, densifier=None) -> None:
        """train.py:103-105, after Adam and densification: drop the rows with ``sigmoid(opacities) < 0.5`` through
        ``densifier.update_state``, which keeps the Adam moments and the densifier's own rows in step (``_rows.compact``
        without a densifier: parameters and moments)."""
        if not self.prune_due(step):
            return
        mask = (torch.sigmoid(model.opacities) < 0.5).reshape(-1)
        if densifier is not None:
            densifier.update_state(optimizer, mask)
        else:
            compact(model, optimizer, mask)

    def terms(self, model, step: int) -> Dict[str, tuple]:
        out = {}
        if self.opacity_active(step):
            out["loss_opacity"] = (float(self.config.lambda_opacity), opacity_entropy(model.opacities))
        return out
