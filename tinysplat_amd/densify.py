"""Densification hooks of tinysplat's GaussianModel on the HIP library.

Host-side mirror of /root/reference/tinysplat/splatting/model_gaussian.py:130-242 - same method
names, argument meaning and gating - over the C-ABI entries of csrc/densify.hip:

    update_grad_accum(step, extras)          :130-132
    reset_opacities(step)                    :134-136
    densify_and_prune(step, optim, extras)   :138-195  (+ GaussianDistribution.sample :533-572)
    update_state(optim, mask, tensors)       :197-242

The model is any holder of the six parameter tensors (synthetic.SplatModel); ``optim`` is
training.Adam (exp_avg / exp_avg_sq dictionaries keyed by parameter name, per-tensor step counts
that densification leaves untouched, as the reference does by carrying the state dict over).
Nothing here falls back to PyTorch indexing: the rebuilt tensors come from ts_gather_rows, through _rows.py.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import TsDensifyPolicy
from ._rows import FIELDS, compact, fields_of, gather, hold, install, plan, rebuild   # noqa: F401 (FIELDS: importable)
from .ops import _call, _f32c, _need_hip, _ptr, _stream

MAX_GAUSSIANS = 1000000          # model_gaussian.py:146


@dataclass
class DensifyConfig:
    """scripts/train.py:206-214 defaults."""
    warmup_densify: int = 600
    warmup_grad: int = 500
    interval_densify: int = 100
    interval_opacity_reset: int = 3000
    densify_end: int = 30000
    epsilon_alpha: float = 0.005
    tau_means: float = 0.0002
    densify_scale_thresh: float = 0.01
    # Not in the reference: after a rebuild, order the rows along a Morton curve of the means
    # (synthetic.morton_order).  The reference appends clones and split samples at the end
    # (model_gaussian.py:179-195), so a trained model's memory order is an accident of its history; the
    # binning scatter and the compositing gathers run measurably faster when neighbours in space are
    # neighbours in memory (5 M Gaussians at 4K, 5.6 -> 4.9 ms per frame).  Off by default:
    # with it the rows are a permutation of the reference's layout.
    spatial_order: bool = False


class Densifier:
    def __init__(self, model, config: Optional[DensifyConfig] = None):
        self.model = model
        self.cfg = config or DensifyConfig()
        self.means_grad_accum = torch.zeros(model.means.shape[0], dtype=torch.float32,
                                            device=model.means.device)      # :62
        self.last_counts = None      # (kept, cloned, split, new total) of the last rebuild
        hold(model, "Densifier")     # see SplatModel.spatial_sort_: the accumulator is per row

    # ------------------------------------------------------------------ :130-132
    @torch.no_grad()
    def update_grad_accum(self, step: int, extras) -> None:
        if step < self.cfg.warmup_grad:
            return
        g = extras["xys"].grad
        if g is None:
            raise RuntimeError("extras['xys'].grad is missing: run backward before update_grad_accum")
        dev = _need_hip(g, self.means_grad_accum)
        g = _f32c(g)
        n = self.means_grad_accum.shape[0]
        if g.shape != (n, 2):
            raise ValueError(f"xys.grad must be [{n}, 2]")
        with torch.cuda.device(dev):
            _call("ts_grad_accum", _lib.load().ts_grad_accum, n, _ptr(g), _ptr(self.means_grad_accum),
                  _stream(dev))

    # ------------------------------------------------------------------ :134-136
    @torch.no_grad()
    def reset_opacities(self, step: int) -> None:
        if step % self.cfg.interval_opacity_reset != 0:
            return
        self.model.opacities.data.fill_(self.cfg.epsilon_alpha / 2)

    # ------------------------------------------------------------------ :138-195
    @torch.no_grad()
    def classify(self, width: int, height: int) -> Tensor:
        """Policy bits per Gaussian (TS_DENSIFY_CLONE | SPLIT | PRUNE), uint8 [N]."""
        m = self.model
        dev = _need_hip(m.scales, m.opacities, self.means_grad_accum)
        n = m.means.shape[0]
        flags = torch.empty((n,), dtype=torch.uint8, device=dev)
        pol = TsDensifyPolicy(float(self.cfg.interval_densify), float(max(width, height)),
                              float(self.cfg.tau_means), float(self.cfg.densify_scale_thresh))
        with torch.cuda.device(dev):
            _call("ts_densify_classify", _lib.load().ts_densify_classify, n, _ptr(self.means_grad_accum),
                  _ptr(_f32c(m.scales.detach())), _ptr(_f32c(m.opacities.detach())), ctypes.byref(pol),
                  _ptr(flags), _stream(dev))
        return flags

    @torch.no_grad()
    def densify_and_prune(self, step: int, optim, extras, z: Optional[Tensor] = None) -> bool:
        """Returns True when the tensors were rebuilt.  ``z``: optional unit normal draws [2S, 3]
        for the split samples (tests pass them to compare with the oracle); drawn on the device
        with torch's generator otherwise."""
        c = self.cfg
        if step < c.warmup_densify or step % c.interval_densify != 0:
            return False
        if step > c.densify_end:
            return False
        if self.model.means.shape[0] > MAX_GAUSSIANS:
            return False
        cam = extras["camera"]
        flags = self.classify(cam["width"], cam["height"])
        self._rebuild(optim, flags, z)
        self.means_grad_accum = torch.zeros(self.model.means.shape[0], dtype=torch.float32,
                                            device=self.model.means.device)        # :195
        if self.cfg.spatial_order:
            self.reorder(optim)
        return True

    @torch.no_grad()
    def reorder(self, optim, perm: Optional[Tensor] = None) -> Tensor:
        """Permutes the rows of the six parameter tensors, both Adam moments and the gradient
        accumulator (default: along a Morton curve of the means, synthetic.morton_order) and returns
        the permutation.  Not in the reference - see DensifyConfig.spatial_order."""
        from .synthetic import morton_order
        m = self.model
        old, live, n, dev = fields_of(m)
        if perm is None:
            perm = morton_order(m.means)
        if perm.shape != (n,):
            raise ValueError(f"perm must be a permutation of the {n} rows")
        src_of = perm.to(device=dev, dtype=torch.int32)
        install(m, optim, *rebuild(old, live, optim, src_of, n, n, n))
        if self.means_grad_accum.shape[0] == n:
            self._gather_accum(src_of, n, dev)
        return perm

    def _gather_accum(self, src_of: Tensor, rows: int, dev) -> None:
        accum = torch.empty((rows,), dtype=torch.float32, device=dev)
        gather([self.means_grad_accum], [accum], rows, rows, src_of, dev)
        self.means_grad_accum = accum

    # ------------------------------------------------------------------ :197-242
    @torch.no_grad()
    def update_state(self, optim, mask: Tensor, _tensors=None) -> None:
        """model_gaussian.py:197-242: drop the rows where ``mask`` is True and append the caller's rows (``_tensors``) -
        ``_rows.compact``, which states the layout and the checks.  ``means_grad_accum`` keeps the surviving rows only
        (``accum[~mask]``, :242 - shorter than the new N until the caller resets it, as in the reference).  The
        prune-only use is train.py:103-105."""
        n = self.model.means.shape[0]
        kept, src_of = compact(self.model, optim, mask, _tensors)
        self.last_counts = (kept, 0, 0, kept)
        if kept < n or self.model.means.shape[0] > kept:           # rows were dropped or appended
            self._gather_accum(src_of, kept, src_of.device)

    # ------------------------------------------------------------------ :138-195
    def _rebuild(self, optim, flags: Tensor, z: Optional[Tensor]) -> None:
        m = self.model
        old, live, n, dev = fields_of(m)
        (K, C, S, n2), src_of = plan(flags, n, dev)
        self.last_counts = (K, C, S, n2)
        if K == n and C == 0 and S == 0:
            return
        new, new_m, new_v = rebuild(old, live, optim, src_of, n2, n2, K)       # kept | cloned | split samples
        if S > 0:
            if z is None:
                z = torch.randn((2 * S, 3), dtype=torch.float32, device=dev)
            z = _f32c(z)
            if z.shape != (2 * S, 3) or z.device != dev:
                raise ValueError(f"z must be [{2 * S}, 3] on {dev}")
            first = K + C
            with torch.cuda.device(dev):
                _call("ts_split_fixup", _lib.load().ts_split_fixup, 2 * S, src_of[first:].data_ptr(),
                      _ptr(old["means"]), _ptr(old["scales"]), _ptr(old["quats"]), _ptr(z),
                      new["means"][first:].data_ptr(), new["scales"][first:].data_ptr(), _stream(dev))
        self._gather_accum(src_of, K, dev)                              # :242
        install(m, optim, new, new_m, new_v)
