"""Per-view appearance: a learnable colour transform per training image between the render and
the loss, so that exposure, white balance and vignetting that change from photo to photo are explained by the transform
and not by floaters.

A view's transform is a bilateral grid of 3x4 affine colour matrices, float32 ``[L, Gh, Gw, 12]``, sliced per pixel by its
position and its luminance (Wang et al., "Bilateral Guided Radiance Field Processing", 2024); a ``(1, 1, 1)`` grid is a
plain per-image exposure matrix.  Every grid starts as the identity, which returns the image bit for bit.  The forward,
the backward, the grid's total variation and the optimiser step are HIP entries (csrc/appearance.hip, ``ts_adam_step``);
nothing here falls back to PyTorch math.  The definition is this project's own: the reference has no appearance model and
parity with other implementations is not pinned.
"""
from __future__ import annotations

import ctypes
from dataclasses import asdict, dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _need_hip, _ptr, _stream

ENTRIES = 12                     # TS_APP_ENTRIES: floats per vertex, entry 4 r + k = element (r, k) of a 3x4 matrix
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


@dataclass
class AppearanceConfig:
    """``grid``: (L, Gh, Gw), luminance levels x grid rows x grid columns; ``(1, 1, 1)`` is one exposure matrix per image.
    ``lr``, ``betas``, ``eps``: Adam on a view's grid; ``tv_weight``: weight of the grid's total variation."""
    grid: Tuple[int, int, int] = (8, 16, 16)
    lr: float = 2e-3
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15
    tv_weight: float = 10.0

    def __post_init__(self):
        self.grid = tuple(int(v) for v in self.grid)
        if len(self.grid) != 3 or min(self.grid) < 1:
            raise ValueError(f"AppearanceConfig: grid = {self.grid} must be three sizes of at least 1")
        if self.lr < 0 or self.tv_weight < 0 or self.eps <= 0:
            raise ValueError("AppearanceConfig: lr and tv_weight must not be negative and eps must be positive")


def _check(image: Tensor, grid: Tensor):
    dev = _need_hip(image, grid)
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.float32:
        raise ValueError("image must be float32 [H, W, 3]")
    if grid.dim() != 4 or grid.shape[3] != ENTRIES or grid.dtype != torch.float32 or not grid.is_contiguous():
        raise ValueError("grid must be a contiguous float32 [L, Gh, Gw, 12] tensor")
    return dev, int(image.shape[0]), int(image.shape[1]), tuple(int(v) for v in grid.shape[:3])


def apply_grid(image: Tensor, grid: Tensor) -> Tensor:
    """``ts_appearance_fwd``: the sliced affine map of every pixel of ``image`` (float32 [H, W, 3]) -> a new [H, W, 3]
    tensor, not clamped.  No autograd."""
    dev, h, w, (L, gh, gw) = _check(image, grid)
    image = image.contiguous()
    out = torch.empty_like(image)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_appearance_fwd", lib.ts_appearance_fwd, h, w, L, gh, gw, _ptr(image), _ptr(grid), _ptr(out), _stream(dev))
    return out


def grid_backward(image: Tensor, grid: Tensor, v_out: Tensor, v_grid: Optional[Tensor] = None):
    """``ts_appearance_bwd``: (d loss / d image, d loss / d grid) from ``v_out`` = d loss / d out.  ``v_grid``: a
    contiguous float32 tensor of the grid's shape to overwrite, or None for a new one.  The same bits on every run."""
    dev, h, w, (L, gh, gw) = _check(image, grid)
    if v_out.shape != image.shape:
        raise ValueError("v_out must have the image's shape")
    image, v_out = image.contiguous(), _f32c(v_out)
    if v_grid is None:
        v_grid = torch.empty_like(grid)
    elif v_grid.shape != grid.shape or v_grid.dtype != torch.float32 or not v_grid.is_contiguous():
        raise ValueError("v_grid must be a contiguous float32 tensor of the grid's shape")
    v_image = torch.empty_like(image)
    lib = _lib.load()
    ws = torch.empty((int(lib.ts_appearance_ws_bytes(h, w, L, gh, gw)),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _call("ts_appearance_bwd", lib.ts_appearance_bwd, h, w, L, gh, gw, _ptr(image), _ptr(grid), _ptr(v_out),
              _ptr(v_image), _ptr(ws), _ptr(v_grid), _stream(dev))
    return v_image, v_grid


def grid_tv(grid: Tensor, weight: float = 1.0, v_in: Optional[Tensor] = None, v_out: Optional[Tensor] = None):
    """``ts_grid_tv``: (tv(grid) as a float64 [1] device tensor, ``v_in + weight * d tv / d grid``).  ``v_out`` may be
    ``v_in`` itself."""
    dev = _need_hip(grid)
    if grid.dim() != 4 or grid.shape[3] != ENTRIES or grid.dtype != torch.float32 or not grid.is_contiguous():
        raise ValueError("grid must be a contiguous float32 [L, Gh, Gw, 12] tensor")
    for t in (v_in, v_out):
        if t is not None and (t.shape != grid.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
            raise ValueError("v_in and v_out must be contiguous float32 tensors of the grid's shape on its device")
    if v_out is None:
        v_out = torch.empty_like(grid)
    value = torch.empty((1,), dtype=torch.float64, device=dev)
    L, gh, gw = (int(v) for v in grid.shape[:3])
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_grid_tv", lib.ts_grid_tv, L, gh, gw, _ptr(grid), float(weight), _ptr(v_in), _ptr(value), _ptr(v_out),
              _stream(dev))
    return value, v_out


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, model, view):
        image = image.contiguous()
        ctx.model, ctx.view = model, view
        ctx.save_for_backward(image)
        return apply_grid(image, model.grids[view])

    @staticmethod
    def backward(ctx, v_out):
        (image,) = ctx.saved_tensors
        model, view = ctx.model, ctx.view
        fresh = model._pending != view
        v_image, v_grid = grid_backward(image, model.grids[view], v_out, model.grad if fresh else None)
        if not fresh:                                    # a second backward of the same view before its step
            model.grad += v_grid
        model._pending = view
        return v_image, None, None


class AppearanceModel:
    """The grids of ``num_views`` training views, ``[V, L, Gh, Gw, 12]``, with Adam's two moments and a step count per
    view.  A training step touches the rendered view's slice, its moments and its count and nothing else; the bias
    correction uses that view's own count."""

    def __init__(self, num_views: int, config: Optional[AppearanceConfig] = None, device="cuda:0"):
        self.config = config if config is not None else AppearanceConfig()
        self.device = torch.device(device)
        if int(num_views) < 1:
            raise ValueError("AppearanceModel: at least one view")
        if self.device.type != "cuda":
            raise RuntimeError("tinysplat_amd ops run only on a HIP (cuda) device. There is deliberately no CPU fallback.")
        shape = (int(num_views), *self.config.grid, ENTRIES)
        self.grids = torch.tensor(IDENTITY, dtype=torch.float32, device=self.device).expand(shape).contiguous()
        self.exp_avg = torch.zeros_like(self.grids)
        self.exp_avg_sq = torch.zeros_like(self.grids)
        self.steps = [0] * int(num_views)
        self.grad = torch.zeros(shape[1:], dtype=torch.float32, device=self.device)     # of the view in _pending
        self._pending: Optional[int] = None
        self.last_tv: Optional[Tensor] = None

    @property
    def num_views(self) -> int:
        return int(self.grids.shape[0])

    def _view(self, view) -> int:
        view = int(view)
        if not 0 <= view < self.num_views:
            raise IndexError(f"view {view} of {self.num_views}")
        return view

    def apply(self, image: Tensor, view: int) -> Tensor:
        """``image`` through view ``view``'s grid; differentiable with respect to ``image``.  The backward pass leaves the
        grid's gradient with the model, for ``step(view)``."""
        view = self._view(view)
        if self._pending is not None and self._pending != view:
            raise RuntimeError(f"the gradient of view {self._pending} is waiting for step({self._pending})")
        return _Apply.apply(image, self, view)

    @torch.no_grad()
    def tv(self, view: int) -> Tensor:
        """tv of the view's grid, a float64 [1] device tensor."""
        return grid_tv(self.grids[self._view(view)])[0]

    @torch.no_grad()
    def step(self, view: int) -> Optional[Tensor]:
        """Adds ``tv_weight`` x the total variation's gradient to the view's pending gradient, applies Adam
        (``ts_adam_step`` on the view's slice, bias-corrected with the view's own count) and clears the gradient.
        -> tv of the grid before the update (float64 [1]); None when no backward pass left a gradient for the view."""
        view = self._view(view)
        if self._pending != view:
            return None
        cfg, dev = self.config, self.device
        grid = self.grids[view]
        value, _ = grid_tv(grid, cfg.tv_weight, self.grad, self.grad)
        self.steps[view] += 1
        one_p, one_l, one_f, one_i = ctypes.c_void_p * 1, ctypes.c_int64 * 1, ctypes.c_float * 1, ctypes.c_int32 * 1
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_adam_step", lib.ts_adam_step, 1, one_p(grid.data_ptr()), one_p(self.grad.data_ptr()),
                  one_p(self.exp_avg[view].data_ptr()), one_p(self.exp_avg_sq[view].data_ptr()), one_l(grid.numel()),
                  one_f(cfg.lr), one_i(self.steps[view]), cfg.betas[0], cfg.betas[1], cfg.eps, _stream(dev))
        self._pending = None
        self.last_tv = value
        return value

    # ---- persistence
    def state_dict(self) -> dict:
        return {"config": asdict(self.config), "grids": self.grids.detach().cpu(), "exp_avg": self.exp_avg.cpu(),
                "exp_avg_sq": self.exp_avg_sq.cpu(), "steps": list(self.steps)}

    def load_state_dict(self, state: dict) -> None:
        if tuple(state["grids"].shape) != tuple(self.grids.shape):
            raise ValueError(f"grids of shape {tuple(state['grids'].shape)} do not fit {tuple(self.grids.shape)}")
        for name in ("grids", "exp_avg", "exp_avg_sq"):
            getattr(self, name).copy_(state[name].to(self.device, torch.float32))
        self.steps = [int(s) for s in state["steps"]]
        self._pending = None

    def save(self, path) -> None:
        torch.save(self.state_dict(), str(path))

    @classmethod
    def load(cls, path, device="cuda:0") -> "AppearanceModel":
        state = torch.load(str(path), map_location="cpu")
        cfg = dict(state["config"])
        cfg["grid"], cfg["betas"] = tuple(cfg["grid"]), tuple(cfg["betas"])
        model = cls(int(state["grids"].shape[0]), AppearanceConfig(**cfg), device)
        model.load_state_dict(state)
        return model
