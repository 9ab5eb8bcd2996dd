"""Training and evaluation masks: which pixels of a photo count as ground truth.

A mask is a ``uint8 [H, W]`` tensor on the device, aligned with a camera's target.  Byte b weighs its pixel by
``m = b / 255``: 255 counts, 0 is ignored, values in between are soft weights (the edges of a binary mask after it went
through the undistortion).  The loss kernels (csrc/train.hip) and the metrics kernel (csrc/metrics.hip) read the bytes
themselves - ``training.photometric_loss(..., mask=)``, ``TrainStep(..., mask=)``, ``fit(..., masks=)``,
``metrics.image_metrics(..., mask=)``, ``evaluate(..., masks=)``.  Here is where masks come from: files beside the photos
(``TrainingMasks``: COLMAP's ``mask_path`` convention) and stored label maps (``masks_from_labels``), and the small
operations on them, which run once per image at load time and are plain tensor expressions.

An ignored target pixel still enters the SSIM statistics of windows up to 10 pixels away (through the target, never
through the render), so a mask of imprecise origin should be grown: ``dilate_ignored``.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

SSIM_REACH = 10                  # pixels: how far an ignored pixel reaches through the 11-tap SSIM window


def as_mask(mask: Tensor) -> Tensor:
    """A mask as the kernels read it: contiguous uint8 [H, W].  A bool tensor becomes 0 / 255."""
    if not isinstance(mask, Tensor) or mask.dim() != 2 or mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError("a mask must be a uint8 or bool [H, W] tensor")
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8) * 255
    return mask.contiguous()


def mask_weights(mask: Tensor) -> Tensor:
    """float32 [H, W]: the weights m = byte / 255 as the kernels' table holds them (the correctly rounded quotient of
    each of the 256 values, computed on the host: on the device torch multiplies by a reciprocal)."""
    mask = as_mask(mask)
    table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(mask.device)
    return table[mask.long()]


def substituted_image(image: Tensor, target: Tensor, mask: Tensor) -> Tensor:
    """``ts_mask_blend``: the image the masked loss reads, written out - ``image`` where the byte is 255, otherwise
    ``fma(m, image - target, target)`` (csrc/mask_math.h), so ``target`` exactly where it is 0.  image, target: float32
    [H, W, 3] on the GPU; mask: uint8 or bool [H, W] -> a new float32 [H, W, 3] tensor."""
    from . import _lib
    from .ops import _call, _need_hip, _ptr, _stream
    mask = as_mask(mask)
    dev = _need_hip(image, target, mask)
    if image.dim() != 3 or image.shape[2] != 3 or image.shape != target.shape or image.dtype != torch.float32 \
            or target.dtype != torch.float32 or tuple(mask.shape) != tuple(image.shape[:2]):
        raise ValueError("image and target must be float32 [H, W, 3] and the mask [H, W]")
    image, target = image.contiguous(), target.contiguous()
    out = torch.empty_like(image)
    h, w = int(image.shape[0]), int(image.shape[1])
    with torch.cuda.device(dev):
        _call("ts_mask_blend", _lib.load().ts_mask_blend, h, w, _ptr(image), _ptr(target), _ptr(mask), _ptr(out), _stream(dev))
    return out


def mask_coverage(mask: Tensor) -> float:
    """The mean weight of a mask: 1.0 keeps everything, 0.0 nothing."""
    mask = as_mask(mask)
    return float(mask.to(torch.float64).mean().item() / 255.0) if mask.numel() else 0.0


def combine_masks(a: Tensor, b: Tensor) -> Tensor:
    """The per-pixel minimum of the bytes: a pixel counts as far as both masks let it."""
    a, b = as_mask(a), as_mask(b)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"masks of one size on one device expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return torch.minimum(a, b)


def dilate_ignored(mask: Tensor, radius: int) -> Tensor:
    """Grows the ignored region by a square of ``radius`` pixels: every byte becomes the minimum of the bytes in its
    (2 radius + 1)^2 window, cut at the image's border.  radius 0 returns the mask.  Once per image at load time: a
    max-pool of the inverted bytes on the mask's device."""
    mask = as_mask(mask)
    radius = int(radius)
    if radius < 0:
        raise ValueError("radius must not be negative")
    if radius == 0 or mask.numel() == 0:
        return mask
    h, w = int(mask.shape[0]), int(mask.shape[1])
    inverted = (255 - mask).to(torch.float32)[None, None]          # 0 .. 255: exact in float32
    # max_pool2d wants padding <= kernel / 2 and pads with -inf (the border cuts the window, as wanted); a radius beyond
    # the image covers all of it anyway, and two passes of one axis each keep the window a square
    ry, rx = min(radius, h), min(radius, w)
    pooled = torch.nn.functional.max_pool2d(inverted, kernel_size=(2 * ry + 1, 1), stride=1, padding=(ry, 0))
    pooled = torch.nn.functional.max_pool2d(pooled, kernel_size=(1, 2 * rx + 1), stride=1, padding=(0, rx))
    return (255 - pooled[0, 0].to(torch.uint8)).contiguous()


def masks_from_labels(semantic_maps, drop_classes: Sequence[int], dilate: int = 0) -> List[Tensor]:
    """One mask per stored label map of ``semantic_maps`` (a ``semantic.SemanticMaps``): 0 where the label is one of
    ``drop_classes`` (in the maps' own label ids), 255 elsewhere - the ignore label included: what the segmenter could
    not name is kept.  ``dilate``: the ignored region is grown by that many pixels (``dilate_ignored``)."""
    drop = sorted({int(c) for c in drop_classes})
    num_classes = int(semantic_maps.num_classes)
    if any(c < 0 or c >= num_classes for c in drop):
        raise ValueError(f"drop_classes must be labels in [0, {num_classes}), got {drop}")
    out = []
    for m in semantic_maps.maps:
        table = torch.full((256,), 255, dtype=torch.uint8, device=m.device)
        if drop:
            table[torch.tensor(drop, dtype=torch.long, device=m.device)] = 0
        out.append(dilate_ignored(table[m.long()], dilate))
    return out


def _read_mask_file(path: str) -> np.ndarray:
    """A mask file -> uint8 [rows, columns], 255 where the file is nonzero (in any channel of an image)."""
    if path.endswith(".npy"):
        a = np.load(path, allow_pickle=False)
        while a.ndim > 2 and a.shape[0] == 1:                      # a batch axis of one
            a = a[0]
    else:
        from PIL import Image as PILImage
        with PILImage.open(path) as f:
            a = np.array(f)
    if a.ndim == 3:
        a = (a != 0).any(axis=2)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{path}: a mask must be [rows, columns], got {tuple(a.shape)}")
    return np.where(a != 0, 255, 0).astype(np.uint8)


class TrainingMasks(Sequence):
    """One mask per camera of ``dataset`` (a ``dataset.Dataset``) read from ``masks_path``: for an image named ``a.jpg``
    the files tried are ``a.jpg.png`` (COLMAP's ``mask_path`` convention), then ``a.png``, then ``a.jpg.npy``; nonzero
    means keep.  A camera without a file raises, and the message lists all of them.  ``masks[i]`` is the uint8 [H, W]
    mask of camera i on ``device``; ``files[i]`` the file it came from.

    A mask of the photo's source size goes where its photo went: where the dataset resampled the photo (undistortion,
    downscaling), the mask, replicated to three channels, goes through ``dataset.undistort_image`` with that camera's own
    intrinsics, and one channel of the uint8 result is the mask - resampled exactly like its photo, soft along its edges.
    A mask already of the camera's size, where the photo was resampled from another size, is used as it is; any other
    size is refused."""

    def __init__(self, dataset, masks_path, device="cuda:0"):
        self.cameras = list(dataset.cameras)
        self.device = torch.device(device)
        self.names = [str(getattr(c, "name", i)) for i, c in enumerate(self.cameras)]
        setups = getattr(dataset, "setups", None)
        sizes = getattr(dataset, "source_sizes", None)
        found: List[Optional[str]] = []
        for name in self.names:
            tried = [name + ".png", os.path.splitext(name)[0] + ".png", name + ".npy"]
            found.append(next((os.path.join(str(masks_path), t) for t in tried
                               if os.path.exists(os.path.join(str(masks_path), t))), None))
        missing = [name for name, path in zip(self.names, found) if path is None]
        if missing:
            raise FileNotFoundError(f"no mask in {masks_path} for: {', '.join(missing)}")
        self.files: List[str] = list(found)
        self.masks: List[Tensor] = []
        for i, (cam, path) in enumerate(zip(self.cameras, self.files)):
            m = _read_mask_file(path)
            h, w = int(cam.height), int(cam.width)
            setup = None if setups is None else setups[i]
            source = None if sizes is None else (int(sizes[i][0]), int(sizes[i][1]))          # (width, height)
            if setup is not None and setup.resample and source == (m.shape[1], m.shape[0]):
                from .dataset import undistort_image
                src = torch.from_numpy(np.ascontiguousarray(np.repeat(m[:, :, None], 3, axis=2))).to(self.device)
                warped = undistort_image(src, setup.src_k, setup.dst_k, setup.dist, setup.out_size)
                self.masks.append(warped[:, :, 0].contiguous())
            elif m.shape == (h, w):
                self.masks.append(torch.from_numpy(np.ascontiguousarray(m)).to(self.device))
            else:
                wanted = f"{h} x {w} (the camera's)" + ("" if source is None else f" or {source[1]} x {source[0]} (the photo's)")
                raise ValueError(f"{path}: a mask of {m.shape[0]} x {m.shape[1]} pixels fits neither size: {wanted}")

    def __len__(self) -> int:
        return len(self.masks)

    def __getitem__(self, i):
        return self.masks[i]


def dataset_masks(dataset, masks_path=None, semantic_path=None, drop_classes: Optional[Sequence[int]] = None,
                  dilate: int = SSIM_REACH, num_classes: int = 150, device="cuda:0") -> Optional[List[Tensor]]:
    """The masks of a dataset's cameras from both sources, as the tools take them: files in ``masks_path``
    (``TrainingMasks``) and the classes ``drop_classes`` of the label maps in ``semantic_path`` (``masks_from_labels``,
    grown by ``dilate`` pixels: the label maps' outlines are a segmenter's), combined per pixel where both are given.
    None where neither is."""
    out = None
    if masks_path is not None:
        out = list(TrainingMasks(dataset, masks_path, device))
    if drop_classes:
        if semantic_path is None:
            raise ValueError("classes to drop need the folder of the label maps")
        from .semantic import SemanticMaps
        labelled = masks_from_labels(SemanticMaps(dataset, semantic_path, num_classes=num_classes, device=device),
                                     drop_classes, dilate)
        out = labelled if out is None else [combine_masks(a, b) for a, b in zip(out, labelled)]
    return out
