"""Semantic labels for the Gaussians: the counterpart of tinysplat/semantic.py.

The reference runs Mask2Former per image, caches its output as ``semantic/<image name>.npy`` (``np.save`` of an int64
[H, W] tensor), reads the files back on the next run and hangs them on the cameras as ``camera.semantic_map``
(semantic.py:9-33); nothing reads the maps after that.  The network stays out of scope.  This module reads maps made with
any model and does what their users want next: it decides which class every Gaussian belongs to, so that a trained
scene can be cut, exported per class and checked against held-out maps.

``votes[g, c]`` is the sum, over all given views and all pixels of column ``c``, of ``rint(2^24 vis_g(p))`` with
``vis_g(p)`` the float32 weight the forward compositing kernel blends Gaussian ``g`` into pixel ``p`` with
(csrc/votes.hip walks the forward's tile lists once per view for all classes at once).  The sums are integers: they do
not depend on the order of views, tiles or calls and are the same bits on every run.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import ops as _ops
from .ops import _call, _need_hip, _ptr, _stream
from .rasterizer import project_args
from .synthetic import SplatModel

NONE = 255                    # TS_VOTE_NONE: the label of a Gaussian or pixel without one; a pixel that does not vote
MAX_CLASSES = 255             # TS_VOTE_MAX_CLASSES
VOTE_SCALE = float(1 << 24)   # TS_VOTE_SCALE


def resample_nearest(label_map: np.ndarray, height: int, width: int) -> np.ndarray:
    """[S_h, S_w] -> [height, width], sampled nearest at pixel centres: ``src = floor((p + 0.5) * S / D)`` per axis, in
    integers."""
    sh, sw = label_map.shape
    rows = ((2 * np.arange(height, dtype=np.int64) + 1) * sh) // (2 * height)
    cols = ((2 * np.arange(width, dtype=np.int64) + 1) * sw) // (2 * width)
    return label_map[rows[:, None], cols[None, :]]


def build_class_map(num_classes: int, classes: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, List[int]]:
    """-> (class_map uint8 [256], class_ids): label -> vote column or 255.  Without ``classes`` label ``l`` votes in
    column ``l``; with it only those labels vote, label ``classes[i]`` in column ``i``."""
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"num_classes must be in 1..{MAX_CLASSES}")
    ids = list(range(int(num_classes))) if classes is None else [int(c) for c in classes]
    if not ids or len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= num_classes:
        raise ValueError(f"classes must be distinct labels in [0, {num_classes})")
    class_map = np.full(256, NONE, dtype=np.uint8)
    class_map[ids] = np.arange(len(ids), dtype=np.uint8)
    return class_map, ids


class SemanticMaps:
    """The label maps of a dataset: reads ``<semantic_path>/<camera.name>.npy`` (the reference's naming,
    semantic.py:33) for every camera of ``dataset_or_cameras`` (a ``Dataset`` or a sequence of cameras) and keeps them
    on ``device`` as uint8 [H, W] tensors in ``maps``, aligned with ``cameras``; ``ignore_label`` is stored as 255.  A
    file must hold an integer [H, W] array (leading axes of one are dropped) with values in ``[0, num_classes)`` or
    ``ignore_label``; a map of another size than the camera is sampled nearest at pixel centres.  ``classes=[...]`` keeps
    only those labels, in that order, as the vote columns: ``votes`` is N x C x 8 bytes, so this is how to lift a few
    classes of many cheaply."""

    def __init__(self, dataset_or_cameras, semantic_path, num_classes: int = 150, ignore_label: int = 255,
                 classes: Optional[Sequence[int]] = None, device="cuda:0"):
        self.cameras = list(getattr(dataset_or_cameras, "cameras", dataset_or_cameras))
        self.num_classes, self.ignore_label = int(num_classes), int(ignore_label)
        class_map, self.class_ids = build_class_map(self.num_classes, classes)
        self.device = torch.device(device)
        self.class_map = torch.from_numpy(class_map).to(self.device)
        self.names = [str(getattr(c, "name", i)) for i, c in enumerate(self.cameras)]
        paths = [os.path.join(str(semantic_path), name + ".npy") for name in self.names]
        missing = [name for name, path in zip(self.names, paths) if not os.path.exists(path)]
        if missing:
            raise FileNotFoundError(f"no semantic map in {semantic_path} for: {', '.join(missing)}")
        self.maps: List[Tensor] = []
        for cam, path in zip(self.cameras, paths):
            m = np.load(path, allow_pickle=False)
            while m.ndim > 2 and m.shape[0] == 1:                      # a batch axis of one
                m = m[0]
            if not np.issubdtype(m.dtype, np.integer):
                raise ValueError(f"{path}: a semantic map must hold integers, got {m.dtype}")
            if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
                raise ValueError(f"{path}: a semantic map must be [rows, columns], got {tuple(m.shape)}")
            ignored = m == self.ignore_label
            bad = ((m < 0) | (m >= self.num_classes)) & ~ignored
            if bad.any():
                raise ValueError(f"{path}: label {int(m[bad].flat[0])} is outside [0, {self.num_classes}) and is not "
                                 f"the ignore label {self.ignore_label}")
            stored = np.where(ignored, NONE, m).astype(np.uint8)
            h, w = int(cam.height), int(cam.width)
            if stored.shape != (h, w):
                stored = resample_nearest(stored, h, w)
            self.maps.append(torch.from_numpy(np.ascontiguousarray(stored)).to(self.device))

    @property
    def num_columns(self) -> int:
        return len(self.class_ids)

    def __len__(self) -> int:
        return len(self.maps)


@dataclass
class LiftResult:
    """``votes`` int64 [N, C]; ``labels`` uint8 [N]: the COLUMN with the most votes, 255 where the Gaussian has none
    (no votes, or its top share is below ``min_share``); ``confidence`` float32 [N]: the top share; ``class_ids``:
    column -> the maps' label."""
    votes: Tensor
    labels: Tensor
    confidence: Tensor
    class_ids: List[int]


def _view_opacity(model, camera, dev):
    """(opacity tensor, TS_RASTER_* flag word) a view of ``model`` composites with: the logits, or for an antialiased model
     the compensated plain opacities of this camera."""
    if _ops.rasterize_mode(model) != "antialiased":
        return model.opacities.detach().contiguous(), _lib.RASTER_LOGIT_OPACITY
    view = camera.view_matrix.to(dev)
    with torch.no_grad():
        o_eff = _ops.compensated_opacity(model, view[:3, :], camera.f_x, camera.f_y, int(camera.width), int(camera.height))
    return o_eff.contiguous(), 0


def _vote_view(model, camera, label_map: Optional[Tensor], class_map: Optional[Tensor], votes: Tensor,
               dummy_colors: Tensor) -> None:
    """Adds one view's votes: project -> bin -> pack -> ts_label_votes, the forward launch's own lists and records."""
    dev = votes.device
    w, h = int(camera.width), int(camera.height)
    n = votes.shape[0]
    xys, depths, radii, conics, nth, _ = _ops.project_gaussians(*project_args(model, camera, (w, h), dev))
    b = _ops.bin_gaussians(xys, depths, radii, nth, h, w, use_cache=False)
    if b.num_intersects == 0:
        return
    opacity, opacity_flags = _view_opacity(model, camera, dev)
    if label_map is not None and (label_map.dtype != torch.uint8 or tuple(label_map.shape) != (h, w)
                                  or label_map.device != dev):
        raise ValueError(f"a label map must be a uint8 [{h}, {w}] tensor on {dev}")
    splats = torch.empty((max(n, 1), 12), dtype=torch.float32, device=dev)
    lib = _lib.load()
    s = _stream(dev)
    with torch.cuda.device(dev):
        _call("ts_pack_splats", lib.ts_pack_splats, n, 3, opacity_flags, _ptr(xys.contiguous()),
              _ptr(b._keep[2]), _ptr(conics.contiguous()), _ptr(dummy_colors), _ptr(opacity),
              _ptr(b.cum_tiles_hit), b.cam, None, _ptr(splats), s)
        _call("ts_label_votes", lib.ts_label_votes, 0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted),
              _ptr(splats), _ptr(None if label_map is None else label_map.contiguous()), _ptr(class_map),
              votes.shape[1], _ptr(votes), s)


@torch.no_grad()
def accumulate_votes(model, cameras: Sequence, maps: Optional[Sequence[Tensor]], class_map: Optional[Tensor],
                     num_columns: int, votes: Optional[Tensor] = None) -> Tensor:
    """``votes`` int64 [N, num_columns] (zeros when not given; accumulated into otherwise) plus the votes of every
    camera.  ``maps``: one uint8 [H, W] device tensor per camera with ``class_map`` uint8 [256], or None for both:
    every pixel votes in column 0."""
    dev = _need_hip(model.means, model.opacities)
    n = int(model.means.shape[0])
    cameras = list(cameras)
    if not 1 <= int(num_columns) <= MAX_CLASSES:
        raise ValueError(f"the number of vote columns must be in 1..{MAX_CLASSES}")
    if (maps is None) != (class_map is None):
        raise ValueError("label maps and a class map go together")
    if maps is not None and len(maps) != len(cameras):
        raise ValueError(f"{len(cameras)} cameras, {len(maps)} label maps")
    if votes is None:
        votes = torch.zeros((n, int(num_columns)), dtype=torch.int64, device=dev)
    elif votes.dtype != torch.int64 or tuple(votes.shape) != (n, int(num_columns)) or not votes.is_contiguous() \
            or votes.device != dev:
        raise ValueError(f"votes must be a contiguous int64 [{n}, {num_columns}] tensor on {dev}")
    if class_map is not None:
        class_map = class_map.to(device=dev, dtype=torch.uint8).contiguous()
        if class_map.numel() != 256:
            raise ValueError("class_map must hold 256 entries")
    dummy = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    for i, camera in enumerate(cameras):
        _vote_view(model, camera, None if maps is None else maps[i], class_map, votes, dummy)
    return votes


def labels_from_votes(votes: Tensor, min_share: float = 0.0) -> Tuple[Tensor, Tensor]:
    """-> (labels uint8 [N], confidence float32 [N]) of int64 [N, C] votes on the GPU: the first largest column where the
    row's sum is positive and ``top >= min_share * sum`` (in double), else 255; ``top / sum``, 0 for an empty row."""
    dev = _need_hip(votes)
    if votes.dtype != torch.int64 or votes.dim() != 2 or not 1 <= votes.shape[1] <= MAX_CLASSES:
        raise ValueError(f"votes must be int64 [N, C] with C in 1..{MAX_CLASSES}")
    votes = votes.contiguous()
    n = int(votes.shape[0])
    labels = torch.empty((n,), dtype=torch.uint8, device=dev)
    confidence = torch.empty((n,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("ts_votes_labels", _lib.load().ts_votes_labels, n, int(votes.shape[1]), _ptr(votes), float(min_share),
              _ptr(labels), _ptr(confidence), _stream(dev))
    return labels, confidence


def lift_labels(model, cameras: Optional[Sequence], maps, min_share: float = 0.0, votes: Optional[Tensor] = None,
                class_map: Optional[Tensor] = None, num_classes: Optional[int] = None) -> LiftResult:
    """Votes of every camera's label map for every Gaussian, and the labels that follow.  ``maps``: a ``SemanticMaps``
    (``cameras`` may then be None: its own; otherwise they are looked up in it by identity, then by name), or a sequence
    of uint8 [H, W] device tensors aligned with ``cameras`` together with ``class_map`` (uint8 [256]: label -> column or
    255) and ``num_classes`` (the number of columns)."""
    if isinstance(maps, SemanticMaps):
        if cameras is None:
            cameras, tensors = maps.cameras, maps.maps
        else:
            cameras, tensors = list(cameras), []
            for cam in cameras:
                hit = [i for i, c in enumerate(maps.cameras) if c is cam] or \
                      [i for i, name in enumerate(maps.names) if name == str(getattr(cam, "name", None))]
                if not hit:
                    raise KeyError(f"camera {getattr(cam, 'name', cam)!r} has no semantic map")
                tensors.append(maps.maps[hit[0]])
        class_map, columns, class_ids = maps.class_map, maps.num_columns, list(maps.class_ids)
    else:
        if class_map is None or num_classes is None:
            raise ValueError("label maps given as tensors need class_map and num_classes")
        tensors, columns, class_ids = list(maps), int(num_classes), list(range(int(num_classes)))
    votes = accumulate_votes(model, cameras, tensors, class_map, columns, votes)
    labels, confidence = labels_from_votes(votes, min_share)
    return LiftResult(votes, labels, confidence, class_ids)


def gaussian_contributions(model, cameras: Sequence) -> Tensor:
    """float64 [N]: every Gaussian's total rendered weight over the cameras' pixels (the one-column, no-map votes
    divided by 2^24) - the importance score of contribution-based pruning."""
    return accumulate_votes(model, cameras, None, None, 1)[:, 0].to(torch.float64) / VOTE_SCALE


def select_gaussians(model, mask: Tensor) -> SplatModel:
    """The Gaussians where ``mask`` (bool [N]) is set, rows in order, as a new model."""
    mask = torch.as_tensor(mask, device=model.means.device)
    if mask.dtype != torch.bool or mask.shape != (model.means.shape[0],):
        raise ValueError("mask must be a bool [N] tensor")
    rows = [p.detach()[mask] for p in model.parameters()]
    return SplatModel(*rows, active_sh_degree=model.active_sh_degree, background=model.background,
                      rasterize_mode=_ops.rasterize_mode(model))


@torch.no_grad()
def render_labels(model, camera, labels: Tensor, num_classes: int) -> Tensor:
    """uint8 [H, W]: per pixel the class whose Gaussians were blended in with the largest summed weight, ties to the
    smaller class, 255 where no class has weight.  ``labels``: uint8 [N], values >= ``num_classes`` carry no class.
    Built on the forward compositing launch with one-hot colours, four classes per pass over the classes that occur."""
    dev = _need_hip(model.means, labels)
    w, h = int(camera.width), int(camera.height)
    n = int(model.means.shape[0])
    if labels.shape != (n,):
        raise ValueError("labels must be [N]")
    present = [int(c) for c in torch.unique(labels).tolist() if int(c) < int(num_classes)]
    out = torch.full((h, w), NONE, dtype=torch.uint8, device=dev)
    if not present:
        return out
    xys, depths, radii, conics, nth, _ = _ops.project_gaussians(*project_args(model, camera, (w, h), dev))
    best = torch.zeros((h, w), dtype=torch.float32, device=dev)
    background = torch.zeros(4, dtype=torch.float32, device=dev)
    opacity, opacity_flags = _view_opacity(model, camera, dev)
    for at in range(0, len(present), 4):                   # ascending classes and a strict `>`: ties to the smaller
        group = present[at:at + 4]
        one_hot = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        for j, c in enumerate(group):
            one_hot[:, j] = (labels == c).to(torch.float32)
        img, _ = _ops.rasterize_gaussians(xys, depths, radii, conics, nth, one_hot, opacity, h, w,
                                          background, logit_opacity=bool(opacity_flags))
        for j, c in enumerate(group):
            better = img[:, :, j] > best
            best = torch.where(better, img[:, :, j], best)
            out = torch.where(better, torch.full_like(out, c), out)
    return out


def label_iou(pred: Tensor, target: Tensor, num_classes: int, ignore: int = 255) -> Tuple[Tensor, float]:
    """-> (iou float64 [num_classes], mean): per class ``|pred = c and target = c| / |pred = c or target = c|`` over the
    pixels whose target is not ``ignore`` (integer counts; NaN where the union is empty), and the mean over the classes
    that occur in the target."""
    pred, target = torch.as_tensor(pred).reshape(-1).to(torch.int64), torch.as_tensor(target).reshape(-1).to(torch.int64)
    if pred.shape != target.shape:
        raise ValueError("pred and target must have the same number of pixels")
    valid = target != int(ignore)
    pred, target = pred[valid], target[valid]
    table = torch.bincount(target * 256 + pred, minlength=256 * 256).reshape(256, 256)[:num_classes]
    inter = table[:, :num_classes].diagonal()
    in_target, in_pred = table.sum(dim=1), torch.bincount(pred, minlength=256)[:num_classes]
    union = in_target + in_pred - inter
    iou = torch.where(union > 0, inter.to(torch.float64) / union.clamp_min(1).to(torch.float64),
                      torch.full((num_classes,), float("nan"), dtype=torch.float64, device=union.device))
    occurs = in_target > 0
    mean = float(iou[occurs].mean()) if bool(occurs.any()) else float("nan")
    return iou, mean
