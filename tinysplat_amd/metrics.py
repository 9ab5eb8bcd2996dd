"""Held-out view evaluation: PSNR, SSIM and L1 of rendered views against their targets.

The reference ends every epoch with a metrics table (scripts/train.py:108-119, :130-149): PSNR (torchmetrics'
``PeakSignalNoiseRatio(data_range=1.0)``, model_gaussian.py:57), the L1 and DSSIM parts of the loss and the number of
Gaussians, averaged over cameras.  Here the table is taken on views held out of training: ``holdout_split`` picks them,
``evaluate`` renders each forward-only and measures it with one HIP entry (csrc/metrics.hip: the frame and the ``uint8``
target are read once, nothing but partial sums is written), ``Evaluator`` is the ``on_step`` callback that does so every
so many steps of ``training.fit``.

SSIM is the training loss's: ``pytorch_msssim.SSIM(data_range=1, size_average=True, channel=3)``, an 11-tap sigma-1.5
window with VALID filtering (the mean runs over the (H-10) x (W-10) map).  The tables of the 3DGS papers use a SSIM whose
window is zero-padded at the image border; that is a different number, usually a little lower.
"""
from __future__ import annotations

import csv
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _call, _need_hip, _ptr, _stream

COLUMNS = ("mse", "l1", "ssim", "psnr")          # the four doubles of ts_image_metrics, in its order


def image_metrics(image: Tensor, target: Tensor, out: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> Tensor:
    """{mse, l1, ssim, psnr} of ``image`` (float32 [H, W, 3 or 4]; a fourth channel, the frame's depth, is ignored)
    against ``target`` ([H, W, 3], float32 or uint8 whose bytes stand for b / 255) -> a float64 [4] device tensor, or
    ``out`` (float64 [4], contiguous: a row of a larger table will do).  A uint8 target gives the same bits as its
    float32 quotients b / 255 (IEEE division, what ``target.to(float32) / 255.0`` is on the host; on the device torch
    multiplies by the reciprocal, one ulp off for some bytes).  Two launches on the current stream, no host
    synchronisation.
    ``mask`` (uint8 or bool [H, W]): the values over the pixels the mask keeps, byte b weighing its
    pixel by m = b / 255: mse and l1 are sums of m (x - y)^2 and m |x - y| over 3 sum m, ssim the SSIM map of the masked
    loss's substituted image weighed by the window centres' m, psnr from that mse.  A mask that keeps nothing gives NaN;
    an all-255 mask the unmasked bytes.  None, the default: the launches as they always were."""
    dev = _need_hip(image, target)
    if image.dim() != 3 or image.shape[2] not in (3, 4) or image.dtype != torch.float32:
        raise ValueError("image must be float32 [H, W, 3] or [H, W, 4]")
    h, w, xs = (int(v) for v in image.shape)
    if tuple(target.shape) != (h, w, 3) or target.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"target must be float32 or uint8 [{h}, {w}, 3], got {target.dtype} {tuple(target.shape)}")
    if h <= 10 or w <= 10:
        raise ValueError("SSIM with an 11-tap window needs H, W > 10")
    if out is None:
        out = torch.empty((4,), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (4,) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float64 [4] tensor on the image's device")
    image, target = image.contiguous(), target.contiguous()
    lib = _lib.load()
    if mask is not None:
        from .masks import as_mask
        mask = as_mask(mask)
        if tuple(mask.shape) != (h, w) or mask.device != dev:
            raise ValueError(f"mask must be uint8 or bool [{h}, {w}] on {dev}, got {tuple(mask.shape)} on {mask.device}")
        ws = torch.empty((int(lib.ts_image_metrics_masked_ws_bytes(h, w)),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _call("ts_image_metrics_masked", lib.ts_image_metrics_masked, h, w, xs, _ptr(image), _ptr(target),
                  int(target.dtype == torch.uint8), _ptr(mask), _ptr(ws), _ptr(out), _stream(dev))
        return out
    ws = torch.empty((int(lib.ts_image_metrics_ws_bytes(h, w)),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _call("ts_image_metrics", lib.ts_image_metrics, h, w, xs, _ptr(image), _ptr(target),
              int(target.dtype == torch.uint8), _ptr(ws), _ptr(out), _stream(dev))
    return out


def affine_fit_sums(image: Tensor, target: Tensor) -> Tensor:
    """``ts_affine_fit_sums``: the 22 sums of the least-squares affine colour fit of ``image`` (float32 [H, W, 3]) to
    ``target`` ([H, W, 3], float32 or uint8 whose bytes stand for b / 255) -> a float64 [22] device tensor: with
    phi = (r, g, b, 1), the ten distinct sums of phi phi^T (rr rg rb r gg gb g bb b 1), then phi_k t_c at 10 + 3 k + c.
    Accumulated in double in a fixed order: the same bits on every run."""
    dev = _need_hip(image, target)
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.float32:
        raise ValueError("image must be float32 [H, W, 3]")
    h, w = int(image.shape[0]), int(image.shape[1])
    if tuple(target.shape) != (h, w, 3) or target.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"target must be float32 or uint8 [{h}, {w}, 3], got {target.dtype} {tuple(target.shape)}")
    image, target = image.contiguous(), target.contiguous()
    lib = _lib.load()
    ws = torch.empty((int(lib.ts_affine_fit_ws_bytes(h, w)),), dtype=torch.uint8, device=dev)
    out = torch.empty((22,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _call("ts_affine_fit_sums", lib.ts_affine_fit_sums, h, w, _ptr(image), _ptr(target),
              int(target.dtype == torch.uint8), _ptr(ws), _ptr(out), _stream(dev))
    return out


FIT_RCOND = 1e-12                # singular values of S below this share of the largest count as zero (a one-colour image)


def affine_fit_solve(sums) -> np.ndarray:
    """The 22 sums -> M = (pinv(S) B)^T, float64 [3, 4]: the affine colour map that takes the image closest to the target
    in the least-squares sense; the minimum-norm one where the image's colours do not span all of (r, g, b, 1)."""
    sums = np.asarray(sums, dtype=np.float64).reshape(22)
    S = np.zeros((4, 4), np.float64)
    S[np.triu_indices(4)] = sums[:10]
    S = S + np.triu(S, 1).T
    B = sums[10:].reshape(4, 3)
    return (np.linalg.pinv(S, rcond=FIT_RCOND, hermitian=True) @ B).T


def affine_color_fit(image: Tensor, target: Tensor) -> np.ndarray:
    """float64 [3, 4]: the least-squares affine colour map from ``image`` to ``target``.  The sums
    are taken on the device, the 4x4 solve on the host: one device-to-host copy of 22 doubles."""
    return affine_fit_solve(affine_fit_sums(image, target).cpu().numpy())


def color_corrected(image: Tensor, target: Tensor) -> Tensor:
    """``image`` (float32 [H, W, 3 or 4]; a fourth channel is dropped) mapped by its own affine fit to ``target``: the fit
    as a 1x1x1 grid through ``ts_appearance_fwd`` -> a new [H, W, 3] tensor."""
    from .appearance import apply_grid
    rgb = image[..., :3].contiguous()
    M = torch.from_numpy(affine_color_fit(rgb, target)).to(torch.float32).reshape(1, 1, 1, 12)
    return apply_grid(rgb, M.to(rgb.device))


@dataclass
class EvalResult:
    """``table``: float64 [V, 4], a row of {mse, l1, ssim, psnr} per view; ``names``: the views' names.  The properties
    are means of the per-view values: the reference's per-camera mean, and the convention of the 3DGS papers (a mean of
    per-view PSNRs, not the PSNR of the mean error).  A view whose mask keeps nothing has NaN in its row (DESIGN.md
    section 6v): the means leave such values out, and ``empty`` names the views with one."""
    table: np.ndarray
    names: List[str]
    empty: List[str] = field(default_factory=list)

    def _mean(self, column: str) -> float:
        values = self.table[:, COLUMNS.index(column)]
        if np.isnan(values).any():                     # views whose mask keeps nothing (NaN if none is left)
            kept = values[~np.isnan(values)]
            return float(kept.mean()) if kept.size else float("nan")
        return float(values.mean())

    @property
    def mse(self) -> float:
        return self._mean("mse")

    @property
    def l1(self) -> float:
        return self._mean("l1")

    @property
    def ssim(self) -> float:
        return self._mean("ssim")

    @property
    def psnr(self) -> float:
        return self._mean("psnr")


def _target(targets, i: int) -> Tensor:
    from .dataset import Targets
    return targets.images_u8[i] if isinstance(targets, Targets) else targets[i]      # the bytes as they are: no float copy


@torch.no_grad()
def evaluate(model, cameras: Sequence, targets, device, background=None, color_correct: bool = False,
             refine_poses: int = 0, pose_config=None, masks=None) -> EvalResult:
    """Renders every camera forward-only (``frame.render_view``, the viewer's path: its image is the training forward's
    bit for bit) on a fixed background - black unless given, the reference model's ``torch.zeros(3)``; the training loop
    draws a random one per step - and measures it against ``targets[i]`` (a ``dataset.Targets``, whose uint8 images are
    read directly, or a sequence of float32 / uint8 [H, W, 3] tensors).  View i fills row i of one [V, 4] device table;
    the only device-to-host copy comes after the last view has been enqueued.  The model is left as found: background,
    SH degree, requires_grad flags, no .grad; no random number is drawn.  ``color_correct``: held-out views have no
    colour grid (appearance.py), so each render is first mapped by its own least-squares affine fit to its target
    (``color_corrected``) and then measured; False, the default: the render is measured as it is.
    ``refine_poses``: after pose training the scene has drifted against the held-out cameras, so each view is first
    aligned to its target by that many steps of ``pose.refine_pose`` (Gaussians frozen, the model untouched bit for bit;
    ``pose_config``: its ``PoseConfig``) and measured from the aligned camera; 0, the default: the cameras as given.
    ``masks``: a sequence indexed like the targets of uint8 or bool [H, W] tensors or None per view (DESIGN.md section
    6v): a masked view is measured over its kept pixels (``image_metrics(..., mask=)``); one whose mask keeps nothing
    gets a NaN row, is left out of the result's means and is named in its ``empty``.  With ``color_correct`` the affine
    fit of a masked view still uses ALL its pixels (a masked fit is not built): ignored content pulls on the fit, only
    the measurement leaves it out.  Pose alignment likewise reads the whole image.  None: the calls as they always were."""
    from .rasterizer import GaussianRasterizer
    dev = torch.device(device)
    cameras = list(cameras)
    if len(cameras) == 0 or len(targets) != len(cameras):
        raise ValueError(f"{len(cameras)} cameras, {len(targets)} targets: evaluation needs one target per camera, at least one")
    if masks is not None and len(masks) != len(cameras):
        raise ValueError(f"{len(masks)} masks for {len(cameras)} cameras: masks needs one entry (or None) per camera")
    render = GaussianRasterizer(model, cameras, device=dev)
    table = torch.empty((len(cameras), 4), dtype=torch.float64, device=dev)
    found = model.background
    model.background = (torch.zeros(3, device=dev) if background is None
                        else torch.as_tensor(background, dtype=torch.float32).to(dev))
    try:
        for i, camera in enumerate(cameras):
            if int(refine_poses) > 0:
                from .pose import refine_pose
                camera, _history = refine_pose(model, camera, _target(targets, i), dev, steps=int(refine_poses),
                                               config=pose_config, appearance_fit=color_correct,
                                               background=model.background)
            image, _extras = render(camera, None, model.active_sh_degree)
            if color_correct:
                image = color_corrected(image, _target(targets, i))
            if masks is None or masks[i] is None:
                image_metrics(image, _target(targets, i), out=table[i])
            else:
                image_metrics(image, _target(targets, i), out=table[i], mask=masks[i])
    finally:
        model.background = found
    names = [str(getattr(c, "name", i)) for i, c in enumerate(cameras)]
    table = table.cpu().numpy()
    if masks is None:
        return EvalResult(table, names)
    return EvalResult(table, names, [n for n, row in zip(names, table) if np.isnan(row).any()])


def holdout_split(names: Sequence[str], every: int = 8, offset: int = 0) -> Tuple[List[int], List[int]]:
    """(train indices, test indices) into ``names``: the cameras sorted by image name, every ``every``-th of them, from
    position ``offset`` on, held out - the LLFF / Mip-NeRF 360 convention (``every=8``).  ``every=0`` holds nothing out.
    Both lists are in name order."""
    every, offset = int(every), int(offset)
    if every < 0 or (every > 0 and not 0 <= offset < every) or (every == 0 and offset != 0):
        raise ValueError(f"holdout_split: every = {every} must not be negative, and offset = {offset} must lie in [0, every)")
    order = sorted(range(len(names)), key=lambda i: (names[i], i))
    test = [i for pos, i in enumerate(order) if every > 0 and pos % every == offset]
    held = set(test)
    return [i for i in order if i not in held], test


class Evaluator:
    """An ``on_step(step, out)`` callback for ``training.fit``: evaluates the held-out views whenever
    ``step % every == 0``, and on demand through ``final(step)``.  ``rows`` keeps (step, N, psnr, ssim, l1) - the
    reference's table line (scripts/train.py:142-149) with held-out means, N the number of Gaussians; ``results`` the
    ``EvalResult`` behind each row.  Every row is handed to ``on_result(row, result)`` if given and appended to
    ``csv_path`` if given (the header is written when the file is created).  ``refine_poses`` / ``pose_config``: as
    ``evaluate``'s - every view is aligned to its image first, which leaves the model untouched, so training with the
    evaluator attached stays what it is without.  ``masks``: as ``evaluate``'s, indexed like the targets: the rows are
    means over the views' kept pixels, and over the views that keep any."""
    HEADER = ("step", "n", "psnr", "ssim", "l1")

    def __init__(self, model, cameras, targets, device, every: int, on_result: Optional[Callable] = None,
                 csv_path=None, background=None, color_correct: bool = False, refine_poses: int = 0, pose_config=None,
                 masks=None):
        if int(every) < 0:
            raise ValueError("Evaluator: every must not be negative (0: only final())")
        self.model, self.cameras, self.targets, self.device = model, list(cameras), targets, device
        self.every, self.on_result, self.background = int(every), on_result, background
        self.color_correct = bool(color_correct)
        self.refine_poses, self.pose_config = int(refine_poses), pose_config
        self.masks = masks                         # indexed like the targets (``evaluate``'s ``masks``)
        self.csv_path = None if csv_path is None else Path(csv_path)
        self.rows: List[tuple] = []
        self.results: List[EvalResult] = []

    @staticmethod
    def format(row) -> str:
        """``Metrics.log``'s line (train.py:144-148): ``key: value | ...``, the count last."""
        step, n, psnr, ssim, l1 = row
        return (f"Step: {step:<10} | PSNR: {psnr:<10.4f} | SSIM: {ssim:<10.4f} | L1: {l1:<10.4f} | "
                f"N: {n:<10}")

    def _evaluate(self, step: int):
        result = evaluate(self.model, self.cameras, self.targets, self.device, self.background,
                          **({"color_correct": True} if self.color_correct else {}),
                          **({"refine_poses": self.refine_poses, "pose_config": self.pose_config}
                             if self.refine_poses > 0 else {}),
                          **({} if self.masks is None else {"masks": self.masks}))
        row = (int(step), int(self.model.means.shape[0]), result.psnr, result.ssim, result.l1)
        self.rows.append(row)
        self.results.append(result)
        if self.csv_path is not None:
            new = not self.csv_path.exists()
            with open(self.csv_path, "a", newline="") as f:
                writer = csv.writer(f)
                if new:
                    writer.writerow(self.HEADER)
                writer.writerow([row[0], row[1], *(repr(float(v)) for v in row[2:])])
        if self.on_result is not None:
            self.on_result(row, result)
        return row

    def __call__(self, step: int, out=None) -> None:
        if self.every > 0 and step % self.every == 0:
            self._evaluate(step)

    def final(self, step: int):
        """The row of ``step``: the one the schedule already took at this step, or a new evaluation."""
        if self.rows and self.rows[-1][0] == int(step):
            return self.rows[-1]
        return self._evaluate(step)
