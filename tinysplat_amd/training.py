"""Training step around the render path.

Mirrors one iteration of /root/reference/scripts/train.py:45-106 without the dataset / viewer /
densification policy: render -> (1 - lambda) L1 + lambda (1 - SSIM) (train.py:58-63), optional depth
L1 (train.py:65-69), backward, Adam on the six parameter groups with the reference's learning rates
(train.py:187-193, model_gaussian.py:112-120).  The photometric loss + its image gradient and the
Adam update are HIP kernels behind the C ABI (csrc/train.hip); nothing here falls back to PyTorch
math for them.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib
from ._rows import hold, tables
from .ops import _call, _f32c, _need_hip, _ptr, _stream
from .scene import Scene

# learning-rate defaults of scripts/train.py:187-193, in the order of SplatModel.parameters()
DEFAULT_LRS = {"means": 0.00016, "colors_dc": 0.0025, "colors_rest": 0.000125, "scales": 0.005,
               "quats": 0.001, "opacities": 0.05}
PARAM_ORDER = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")


def _mask_arg(mask, h: int, w: int, dev) -> Tensor:
    """A loss function's ``mask`` as the kernels read it: contiguous uint8 [H, W] on ``dev`` (masks.as_mask: bool -> 0 / 255)."""
    from .masks import as_mask
    mask = as_mask(mask)
    if tuple(mask.shape) != (h, w) or mask.device != dev:
        raise ValueError(f"mask must be uint8 or bool [{h}, {w}] on {dev}, got {tuple(mask.shape)} on {mask.device}")
    return mask


def planes_loss_and_gradient(image: Tensor, depth: Optional[Tensor], target: Tensor, depth_target: Optional[Tensor],
                             lambda_dssim: float, lambda_depth: float, want_rgb: bool = True, want_depth: bool = True,
                             mask: Optional[Tensor] = None):
    """train.py:58-69 in one pair of launches and the reduce, WITHOUT autograd, on any of the three layouts of a frame:
    ``image`` [H,W,3] with ``depth`` None (no depth term), the adapter's two planes as it hands them out (image [H,W,3]
    and depth [H,W], both contiguous: frame.render_frame_planes), or its contiguous [H,W,4] output whose channel 3 is the
    depth (``depth`` None).  -> (values[4] = {loss, l1, ssim, depth l1}, dloss/dimage in the layout of ``image`` or None,
    dloss/ddepth as a plane or None).  ``TrainStep`` hands the two gradients straight to ``torch.autograd.backward`` -
    no loss node, no ``grad * 1.0`` passes over 33 MB.
    ``mask`` (uint8 or bool [H, W]): the masked pair of launches - the loss of the substituted
    image, gradients times the pixel's weight; None: the launches as they always were."""
    dev = _need_hip(image, target) if depth is None else _need_hip(image, depth, target)
    if image.dim() != 3 or image.shape[2] not in (3, 4) or (depth is not None and image.shape[2] != 3):
        raise ValueError("image must be [H, W, 3], or [H, W, 4] (RGB + depth) without a separate depth plane")
    h, w, floats = image.shape
    if (floats == 4 or depth is not None) and not (image.is_contiguous() and (depth is None or depth.is_contiguous())):
        raise ValueError("an [H, W, 4] frame, and an [H, W, 3] image with its [H, W] depth plane, must be contiguous")
    if (target.shape != (h, w, 3) or (depth is not None and depth.shape != (h, w))
            or (depth_target is not None and depth_target.shape != (h, w))):
        raise ValueError("target must be [H, W, 3], depth and depth_target [H, W]")
    if h <= 10 or w <= 10:
        raise ValueError("SSIM with an 11-tap window needs H, W > 10")
    image, target = _f32c(image.detach()), _f32c(target)
    depth = None if depth is None else _f32c(depth.detach())
    dt = None if depth_target is None else _f32c(depth_target)
    lib = _lib.load()
    ws = torch.empty((int(lib.ts_photometric_ws_floats(h, w)),), dtype=torch.float32, device=dev)
    v_image = torch.empty_like(image) if want_rgb else None
    v_depth = torch.empty_like(depth) if (depth is not None and v_image is not None and want_depth and dt is not None) else None
    ho, wo = h - 10, w - 10
    lam, lamd = float(lambda_dssim), float(lambda_depth) if dt is not None else 0.0
    w_l1, w_ssim, w_depth = (1.0 - lam) / (3.0 * h * w), -lam / (3.0 * ho * wo), lamd / (h * w)
    values = torch.empty((4,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        m = None if mask is None else _mask_arg(mask, h, w, dev)
        loss = _lib.TsLoss(height=h, width=w, pixel_floats=floats, flags=0 if m is None else _lib.LOSS_MASKED,
                           image=_ptr(image), depth=_ptr(depth), target=_ptr(target), depth_target=_ptr(dt), mask=_ptr(m),
                           w_l1=w_l1, w_ssim=w_ssim, w_depth=w_depth, ws=_ptr(ws), v_image=_ptr(v_image),
                           v_depth=_ptr(v_depth))
        _call("ts_photometric_loss_rgbd", lib.ts_photometric_loss_rgbd, ctypes.byref(loss), _stream(dev))
        # {loss, l1, ssim, depth l1} as ONE four-float device tensor from the partial sums in ``ws`` (ABI 8: one launch
        # instead of a dozen one-element tensor operations between the loss kernels and the frame's backward pass)
        _call("ts_photometric_loss_reduce", lib.ts_photometric_loss_reduce, h, w, w_l1, w_ssim, w_depth, _ptr(ws),
              _ptr(values), _stream(dev))
    return values, v_image, v_depth


class _Loss(torch.autograd.Function):
    """``planes_loss_and_gradient`` as a differentiable function of the image and, where there is one, the depth plane."""

    @staticmethod
    def forward(ctx, image, depth, target, depth_target, lambda_dssim, lambda_depth, mask):
        values, v_image, v_depth = planes_loss_and_gradient(image, depth, target, depth_target, lambda_dssim, lambda_depth,
                                                            ctx.needs_input_grad[0], ctx.needs_input_grad[1], mask)
        loss, l1, ssim, ldepth = values.unbind(0)
        ctx.has_depth = v_depth is not None
        ctx.save_for_backward(*(t for t in (v_image, v_depth) if t is not None))
        ctx.mark_non_differentiable(l1, ssim, ldepth)
        return loss, l1, ssim, ldepth

    @staticmethod
    def backward(ctx, v_loss, *_):
        saved = ctx.saved_tensors
        v_image = saved[0] * v_loss if saved else None           # out of place: retain_graph re-runs this (train.py:71)
        v_depth = saved[1] * v_loss if ctx.has_depth else None   # None: no depth target, the kernels take "no gradient"
        return v_image, v_depth, None, None, None, None, None


def _need_floats(image: Tensor, floats: int, what: str) -> None:
    if image.dim() != 3 or image.shape[2] != floats:
        raise ValueError(f"{what} must be a [H, W, {floats}] tensor")


def planes_loss(rgb: Tensor, depth: Tensor, target: Tensor, depth_target: Optional[Tensor] = None,
                lambda_dssim: float = 0.2, lambda_depth: float = 0.2, mask: Optional[Tensor] = None):
    """``frame_loss`` on the frame as two planes: ``(loss, l1, ssim, depth_l1)``, differentiable w.r.t. ``rgb`` and
    ``depth``.  ``mask``: as ``photometric_loss``'s."""
    _need_floats(rgb, 3, "rgb")
    if depth is None:
        raise ValueError("planes_loss needs the depth plane; photometric_loss is the loss without one")
    return _Loss.apply(rgb, depth, target, depth_target, lambda_dssim, lambda_depth, mask)


def frame_loss(frame: Tensor, target: Tensor, depth_target: Optional[Tensor] = None,
               lambda_dssim: float = 0.2, lambda_depth: float = 0.2, mask: Optional[Tensor] = None):
    """Total training loss of train.py:58-69 on the adapter's [H, W, 4] output (RGB already clamped,
    channel 3 = depth): ``(1-l) L1 + l (1 - SSIM) [+ l_depth * mean|depth - depth_target|]``.
    Returns ``(loss, l1, ssim, depth_l1)``; differentiable w.r.t. ``frame``.  ``mask``: as ``photometric_loss``'s; the
    depth term becomes ``mean(m |depth - depth_target|)``."""
    _need_floats(frame, 4, "frame")
    return _Loss.apply(frame, None, target, depth_target, lambda_dssim, lambda_depth, mask)


def photometric_loss(image: Tensor, target: Tensor, lambda_dssim: float = 0.2, mask: Optional[Tensor] = None):
    """``(1 - lambda) * mean|image - target| + lambda * (1 - SSIM(image, target))`` on HWC images
    (the loss of train.py:58-63).  Returns ``(loss, l1, ssim)``; differentiable w.r.t. ``image``.
    ``mask`` (uint8 or bool [H, W] on the image's device): byte b weighs its pixel by m = b / 255.
    The loss is then the same loss, with the same weights (not renormalised by the mask's area), of the substituted image
    ``m image + (1 - m) target``, and the gradient is m times that loss's: an ignored pixel (0) gets exactly zero, an
    all-255 mask gives the unmasked bits.  None, the default: the launches as they always were."""
    _need_floats(image, 3, "image")
    return _Loss.apply(image, None, target, None, lambda_dssim, 0.0, mask)[:3]


class Adam:
    """torch.optim.Adam (defaults) over the six parameter tensors, one HIP launch per step."""

    def __init__(self, params: Dict[str, Tensor], lrs: Optional[Dict[str, float]] = None,
                 betas=(0.9, 0.999), eps: float = 1e-8):
        self.names = [n for n in PARAM_ORDER if n in params] + [n for n in params if n not in PARAM_ORDER]
        if len(self.names) > 8:
            raise ValueError("at most 8 tensors per Adam table")
        self.params = {n: params[n] for n in self.names}
        self.lrs = dict(DEFAULT_LRS)
        if lrs:
            self.lrs.update(lrs)
        self.betas, self.eps = betas, eps
        self.steps = {n: 0 for n in self.names}       # per tensor, as torch.optim.Adam's state['step']
        self.exp_avg = {n: torch.zeros_like(p) for n, p in self.params.items()}
        self.exp_avg_sq = {n: torch.zeros_like(p) for n, p in self.params.items()}
        self.fused_steps, self._fused_pending = 0, False

    @torch.no_grad()
    def step(self) -> None:
        with_grad = [n for n in self.names if self.params[n].grad is not None]
        names = [n for n in with_grad if self.params[n].numel() > 0]   # (colors_rest of an SH-0 model: nothing to update)
        ps = [self.params[n] for n in names]
        for p in ps:
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise ValueError("Adam parameters must be contiguous float32")
        gs = [_f32c(p.grad) for p in ps]
        for n in with_grad:
            self.steps[n] += 1
        if not names:
            return
        dev = _need_hip(*ps)
        k = len(names)
        pp, gp, mp, vp, _ = tables(ps, gs, [self.exp_avg[n] for n in names], [self.exp_avg_sq[n] for n in names])
        with torch.cuda.device(dev):
            _call("ts_adam_step", _lib.load().ts_adam_step, k, pp, gp, mp, vp, (ctypes.c_int64 * k)(*[p.numel() for p in ps]),
                  (ctypes.c_float * k)(*[self.lrs.get(n, 1e-3) for n in names]),
                  (ctypes.c_int32 * k)(*[self.steps[n] for n in names]), self.betas[0], self.betas[1], self.eps,
                  _stream(dev))

    def zero_grad(self) -> None:
        for p in self.params.values():
            p.grad = None

    # ---- FUSED ADAM (frame.fused_adam; csrc/project.hip): the frame's backward pass applies this optimiser's update itself
    def fused_begin(self, tensors):
        """Called by the frame's backward pass with the six tensors the frame rendered from, in the order (means,
        scales, quats, opacities, colors_dc, colors_rest).  -> the ``ts_adam`` struct for ts_frame_bwd_params_adam with
        every group's step advanced, or None when these are not this optimiser's own (contiguous float32) tensors."""
        order = ("means", "scales", "quats", "opacities", "colors_dc", "colors_rest")
        if any(n not in self.params for n in PARAM_ORDER):
            return None
        for n, t in zip(order, tensors):
            p = self.params[n]
            if t.data_ptr() != p.data_ptr() or t.shape != p.shape or not p.is_contiguous() or p.dtype != torch.float32:
                return None
        a = _lib.TsAdam()
        for k, n in enumerate(PARAM_ORDER):
            self.steps[n] += 1
            a.exp_avg[k], a.exp_avg_sq[k] = self.exp_avg[n].data_ptr(), self.exp_avg_sq[n].data_ptr()
            a.lr[k], a.step[k] = self.lrs.get(n, 1e-3), self.steps[n]
        a.beta1, a.beta2, a.eps = self.betas[0], self.betas[1], self.eps
        self.fused_steps += 1
        self._fused_pending = True
        return a

    def consume_fused(self) -> bool:
        """True once after a backward pass that applied the update itself (the caller then skips ``step()``)"""
        done, self._fused_pending = self._fused_pending, False
        return done


class TrainStep:
    """render -> loss -> backward -> Adam, one call per iteration (train.py:45-106 minus policy)."""

    def __init__(self, model, device, lambda_dssim: float = 0.2, lambda_depth: float = 0.2,
                 lrs: Optional[Dict[str, float]] = None, scene: Optional[Scene] = None, fused_adam: bool = True):
        self.model, self.device = model, torch.device(device)
        self.lambda_dssim, self.lambda_depth = lambda_dssim, lambda_depth
        # the reference's loop renders through scene.render(camera) (train.py:55 -> scene.py:222-223)
        self.scene = scene if scene is not None else Scene([], model, device=self.device)
        self.rasterizer = self.scene.rasterizer
        model.requires_grad_(True)
        self.optimizer = Adam({n: getattr(model, n) for n in PARAM_ORDER}, lrs)
        # fused_adam: the frame's backward pass applies the Adam update to the gradients it holds in registers (the same
        # update, bit for bit: tests/test_gpu_training.py) and no parameter gradient tensor is written - model.<p>.grad
        # stays None, extras['xys'].grad is set as always.  False: backward, then one ts_adam_step launch.
        self.fused_adam = bool(fused_adam)
        hold(model, "TrainStep")       # per-row state now exists outside the model: see SplatModel.spatial_sort_

    def __call__(self, camera, target_rgb: Tensor, target_depth: Optional[Tensor] = None,
                 densifier=None, step: Optional[int] = None, surface=None, appearance=None, view: Optional[int] = None,
                 poses=None, mask: Optional[Tensor] = None):
        """``densifier`` (densify.Densifier) + ``step`` add train.py:99-102 after the Adam update:
        gradient accumulation and, on the policy's steps, clone / split / prune.  A densifier with a ``loss_terms(model,
        step)`` method (mcmc.McmcDensifier) adds its terms to the loss as ``surface`` does.
        ``surface`` (surface.SurfaceRegularizer) + ``step`` add the regularisers of train.py:71-91 that its schedule
        makes active at ``step`` (the density term on the rendered depth): ``loss += lambda * term``, one backward for
        the whole loss, then the two-launch Adam (the fused in-backward update only sees the frame's own gradients);
        after densification, the prune of train.py:103-105 on its step.  On a step where nothing is active the step
        is exactly the one without ``surface``.
        ``appearance`` (appearance.AppearanceModel) + ``view`` (the camera's index among the training views) put the
        view's colour grid between the render and the loss: the loss reads ``appearance.apply(rgb, view)``, the backward
        pass goes through it into the frame, and ``appearance.step(view)`` updates the view's grid after it; ``out`` gains
        ``appearance_tv``.  The fused in-backward Adam of the Gaussians stays on.  None: the step is exactly today's.
        ``poses`` (pose.PoseModel) + ``view`` render ``poses.camera(view)`` in place of ``camera`` and refine that view's
        pose: the backward pass writes the gradient tensors (the two-launch Adam: the fused update
        keeps no rows to reduce), ``ts_pose_grad`` reduces the rows of means and quats before Adam moves them, and
        ``poses.step(view, g)`` follows; ``out`` gains ``pose_grad``.  A SuGaR density term active at ``step`` is refused:
        its gradient on the means did not come through the camera.  None: the step is exactly today's.
        ``mask`` (uint8 or bool [H, W], aligned with ``target_rgb``) leaves pixels out of the loss:
        whichever of the three loss paths the render selects runs its masked launches, on the image after ``appearance``;
        everything else, the fused Adam included, is as without.  None: the step is exactly today's."""
        masked = {} if mask is None else {"mask": mask}
        if appearance is not None and view is None:
            raise ValueError("appearance needs the index of the rendered view")
        if poses is not None:
            if view is None:
                raise ValueError("poses needs the index of the rendered view")
            if surface is not None and step is not None and surface.density_active(step):
                raise ValueError("poses cannot be refined while the SuGaR density term is active: it puts gradient on the "
                                 "means that did not come through the camera and would enter the pose gradient")
            camera = poses.camera(view)
        terms = {}
        if surface is not None:
            if step is None:
                raise ValueError("the surface regularisers need the 1-based step number")
            terms = surface.terms(self.model, step)
        if densifier is not None and hasattr(densifier, "loss_terms"):   # mcmc.McmcDensifier: its two mean regularisers
            if step is None:
                raise ValueError("densification needs the 1-based step number")
            terms.update(densifier.loss_terms(self.model, step))
        rgb, extras = self.scene.render(camera)
        if surface is not None:                                # train.py:77-91: the density term reads the render
            terms.update(surface.frame_terms(self.model, step, camera, extras))
        frame = getattr(rgb, "_base", None)
        depth = extras["depth"]
        direct = None
        # the image the loss reads; which of the three paths runs is decided on the render, as without appearance
        shown = rgb if appearance is None else appearance.apply(rgb, view)
        if (rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.is_contiguous() and rgb.is_cuda and depth.is_contiguous()
                and depth.shape == rgb.shape[:2] and frame is None):
            # the adapter's one-node path hands out two contiguous images: the whole loss (train.py:58-69) on
            # them in one pair of launches, gradients back as two planes
            values, v_rgb, v_depth = planes_loss_and_gradient(shown, depth, target_rgb, target_depth, self.lambda_dssim,
                                                              self.lambda_depth, **masked)
            loss, l1, ssim, depth_l1 = values.unbind(0)
            direct = ([shown] + ([depth] if v_depth is not None else []), [v_rgb] + ([v_depth] if v_depth is not None else []))
        elif (frame is not None and frame.dim() == 3 and frame.shape[2] == 4 and frame.is_contiguous()
                and extras["depth"]._base is frame):
            # the adapter's one-node path hands out views of ONE [H, W, 4] tensor: evaluate the
            # whole loss (train.py:58-69) on it in place, no slicing / re-packing of image or gradient
            if appearance is None:
                loss, l1, ssim, depth_l1 = frame_loss(frame, target_rgb, target_depth, self.lambda_dssim,
                                                      self.lambda_depth, **masked)
            else:                                              # the applied image is a tensor of its own: the two-plane loss
                loss, l1, ssim, depth_l1 = planes_loss(shown, extras["depth"].contiguous(), target_rgb, target_depth,
                                                       self.lambda_dssim, self.lambda_depth, **masked)
        else:
            loss, l1, ssim = photometric_loss(shown, target_rgb, self.lambda_dssim, **masked)
            if target_depth is not None and mask is not None:     # m |d - D|: the mean still runs over all pixels
                from .masks import mask_weights
                depth_l1 = (mask_weights(mask) * (extras["depth"] - target_depth)).abs().mean()
                loss = loss + self.lambda_depth * depth_l1
            elif target_depth is not None:                        # train.py:65-69
                depth_l1 = (extras["depth"] - target_depth).abs().mean()
                loss = loss + self.lambda_depth * depth_l1
        if terms:                                              # train.py:71-75: loss += lambda * term
            extra = None
            for weight, term in terms.values():
                extra = weight * term if extra is None else extra + weight * term
            if direct is not None:
                direct = (direct[0] + [extra], direct[1] + [None])
            loss = loss + extra
        # `direct`: the loss launches already produced dloss / d(rgb, depth) - they go straight into the frame's backward
        run_backward = (lambda: torch.autograd.backward(*direct)) if direct is not None else loss.backward
        pose_grad = None
        if self.fused_adam and not terms and poses is None:
            from .frame import fused_adam
            with fused_adam(self.optimizer):
                run_backward()
            if not self.optimizer.consume_fused():          # a render path without the one-node frame: the two-launch step
                self.optimizer.step()
        else:
            run_backward()
            if poses is not None:                              # the rows of this frame, before Adam moves means and quats
                from .pose import pose_gradient
                pose_grad = pose_gradient(self.model, camera)
            self.optimizer.step()
        if poses is not None:
            poses.step(view, pose_grad)
        appearance_tv = None if appearance is None else appearance.step(view)
        xys_grad = extras["xys"].grad                          # consumed by densification (F2)
        if densifier is not None:
            if step is None:
                raise ValueError("densification needs the 1-based step number")
            densifier.update_grad_accum(step, extras)         # train.py:101
            densifier.densify_and_prune(step, self.optimizer, extras)   # train.py:102
        if surface is not None:
            surface.after_step(self.model, step, self.optimizer, densifier)   # train.py:103-105
        self.optimizer.zero_grad()
        out = {"loss": loss.detach(), "l1": l1, "ssim": ssim, "radii": extras["radii"], "xys_grad": xys_grad}
        if target_depth is not None:                           # the depth term's value, mean |depth - target|
            out["depth_l1"] = depth_l1.detach()
        for name, (_, term) in terms.items():
            out[name] = term.detach()
        if appearance_tv is not None:
            out["appearance_tv"] = appearance_tv
        if pose_grad is not None:
            out["pose_grad"] = pose_grad
        return out


class Scheduler:
    """scripts/train.py:152-159."""

    def __init__(self, active: bool, start: int, stop: int):
        self.active, self.start, self.stop = active, start, stop

    def __call__(self, step: int) -> bool:
        return bool(self.active) and self.start <= step < self.stop


class CameraSampler:
    """Scene.get_random_camera (scene.py:207-216), condition for condition: a fresh permutation is
    drawn whenever ``step % len(cameras) - 1`` is non-zero (i.e. on every step except those with
    ``step % n == 1``), otherwise the cursor advances.  ``rng``: a numpy Generator (the reference
    uses an unseeded one)."""

    def __init__(self, num_cameras: int, rng=None):
        import numpy as np
        self.n = int(num_cameras)
        self.rng = rng if rng is not None else np.random.default_rng()
        self.order, self.cursor = None, 0

    def __call__(self, step: int) -> int:
        if step % self.n - 1 or self.order is None:
            self.order, self.cursor = self.rng.permutation(self.n), 0
        else:
            self.cursor += 1
        return int(self.order[self.cursor % self.n])


def fit(model, cameras, targets, device, max_iter: int, depth_targets=None,
        sh_increment_interval: int = 500, max_sh_degree: int = 3, lambda_dssim: float = 0.2,
        lambda_depth: float = 0.2, depth_schedule: Optional[Scheduler] = None, densifier=None,
        lrs: Optional[Dict[str, float]] = None, rng=None, generator: Optional[torch.Generator] = None,
        on_step=None, surface=None, lr_schedule=None, appearance=None, poses=None, masks=None):
    """The training loop of scripts/train.py:45-106 (steps 1-7) on in-memory cameras / targets:
    SH degree schedule (:49-50, model_gaussian.py:126-128), random background (:51), camera pick
    (:54), render + loss (:55-69), the opacity-entropy (:71-75) and SuGaR density (:77-91)
    regularisers when ``surface`` (surface.SurfaceConfig) enables them, backward + Adam (:93-97),
    gradient accumulation and densification (:99-102), the density window's opening prune
    (:103-105).  ``generator`` also draws the density samples.  Dataset loading, metrics and
    checkpoints stay with the caller (``on_step(step, out)``).  ``lr_schedule``: a callable ``step -> {name: lr}`` whose
    rates are written into ``Adam.lrs`` before the step (``mcmc.ExponentialLr``: the reference's ``update_learning_rate``
    TODO, model_gaussian.py:122-124); None, the default: the rates stay constant.  ``appearance``: an
    ``appearance.AppearanceConfig`` (a model with one grid per camera is made from it) or an ``AppearanceModel``: every
    step goes through the picked camera's colour grid; None, the default: no colour model.
    ``poses``: a ``pose.PoseConfig`` (a ``PoseModel`` over ``cameras`` is made from it) or a ``PoseModel``: every step
    renders the picked view's refined camera and updates its pose; not together with a SuGaR
    density window that opens within ``max_iter``; None, the default: the cameras are taken as exact.
    ``masks``: a sequence aligned with ``cameras`` (a ``masks.TrainingMasks`` will do) of uint8 or bool [H, W] tensors or
    None per view: the pixels each view's loss leaves out; None, the default, and a view whose
    entry is None: the step as it always was."""
    if masks is not None and len(masks) != len(cameras):
        raise ValueError(f"{len(masks)} masks for {len(cameras)} cameras: masks needs one entry (or None) per camera")
    dev = torch.device(device)
    scene = Scene(cameras, model, device=dev, rng=rng)
    step_fn = TrainStep(model, dev, lambda_dssim, lambda_depth, lrs, scene=scene)
    if surface is not None:
        from .surface import SurfaceRegularizer
        surface = SurfaceRegularizer(surface, generator)
    if appearance is not None:
        from .appearance import AppearanceConfig, AppearanceModel
        if isinstance(appearance, AppearanceConfig):
            appearance = AppearanceModel(len(cameras), appearance, dev)
        if appearance.num_views != len(cameras):
            raise ValueError(f"the appearance model has {appearance.num_views} views, the run {len(cameras)} cameras")
    if poses is not None:
        from .pose import PoseConfig, PoseModel
        if isinstance(poses, PoseConfig):
            poses = PoseModel(cameras, poses)
        if poses.num_views != len(cameras):
            raise ValueError(f"the pose model has {poses.num_views} views, the run {len(cameras)} cameras")
        sc = None if surface is None else surface.config
        if sc is not None and sc.regularize_density and max(1, sc.regularize_density_start) < min(int(max_iter) + 1, sc.regularize_density_end):
            raise ValueError("poses cannot be refined in a run whose SuGaR density term becomes active: it puts gradient "
                             "on the means that did not come through the camera")
    # what a step takes beside the index of its view; empty: the step is called as it always was
    per_view = {k: v for k, v in (("appearance", appearance), ("poses", poses)) if v is not None}
    pick = scene._sampler
    out = None
    for step in range(1, int(max_iter) + 1):
        if step % sh_increment_interval == 0 and model.active_sh_degree < max_sh_degree:
            model.active_sh_degree += 1
        model.background = torch.rand(3, generator=generator).to(dev) if generator is not None \
            else torch.rand(3, device=dev)
        i = pick(step)
        use_depth = depth_targets is not None and (depth_schedule is None or depth_schedule(step))
        if lr_schedule is not None:
            step_fn.optimizer.lrs.update(lr_schedule(step))
        out = step_fn(cameras[i], targets[i], depth_targets[i] if use_depth else None,
                      densifier=densifier, step=step, surface=surface,
                      **per_view, **({} if not per_view else dict(view=i)),
                      **({} if masks is None or masks[i] is None else dict(mask=masks[i])))
        if on_step is not None:
            on_step(step, out)
    return out
