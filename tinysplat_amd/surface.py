"""Surface regularisers of the training loop (scripts/train.py:71-75): the opacity entropy.

``opacity_entropy`` is ``-mean(o log(o + 1e-10) + (1 - o) log(1 - o + 1e-10))`` with ``o = sigmoid(opacities)``,
value and gradient in one C-ABI call (csrc/surface.hip).  ``SurfaceConfig`` holds the reference's command-line
defaults for it (train.py:201, :234-236) and ``SurfaceRegularizer`` its schedule (train.py:33-35, :152-159);
``training.TrainStep`` / ``training.fit`` take one with ``surface=``.  There is no CPU fallback: tensors must be on
the GPU.  The SuGaR density / SDF regulariser (train.py:77-91) is not implemented here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import torch
from torch import Tensor

from . import _lib
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


@dataclass
class SurfaceConfig:
    """The reference's regulariser options (scripts/train.py:201, :234-236) with their command-line defaults:
    ``--regularize-opacity`` (off unless given), ``--lambda-opacity 0.2``, window steps [7000, 9000)."""
    regularize_opacity: bool = False
    lambda_opacity: float = 0.2
    regularize_opacity_start: int = 7000
    regularize_opacity_end: int = 9000


class SurfaceRegularizer:
    """The schedule of train.py:33-35 (``Scheduler``: active for ``start <= step < end`` when enabled) around
    ``opacity_entropy``.  ``terms(model, step)`` -> ``{name: (weight, differentiable scalar)}`` for the terms active
    at ``step`` (empty on every other step)."""

    def __init__(self, config: SurfaceConfig = None):
        self.config = config if config is not None else SurfaceConfig()

    def opacity_active(self, step: int) -> bool:
        c = self.config
        return bool(c.regularize_opacity) and c.regularize_opacity_start <= step < c.regularize_opacity_end

    def active(self, step: int) -> bool:
        return self.opacity_active(step)

    def terms(self, model, step: int) -> Dict[str, tuple]:
        out = {}
        if self.opacity_active(step):
            out["loss_opacity"] = (float(self.config.lambda_opacity), opacity_entropy(model.opacities))
        return out
