"""The three differentiable callables tinysplat imports from gsplat, served by the HIP library.

Signatures are exactly those tinysplat uses (gsplat 0.1.x functional API):

    project_gaussians   /root/reference/tinysplat/splatting/rasterize.py:32  (13 positional args, 6 returns)
    spherical_harmonics rasterize.py:38                                      (3 args, 1 return)
    rasterize_gaussians rasterize.py:44,50                                   (10 args, 2-tuple return)
    num_sh_bases / deg_from_sh   rasterize.py:76, model_gaussian.py:71,106

Every op runs on the HIP device of its inputs, on torch's current stream, through the C ABI of
include/tinysplat_hip.h.  There is NO CPU path and NO PyTorch fallback: CPU tensors raise, and a
missing libtinysplat_hip.so raises at the first call.
"""
from __future__ import annotations

import os
import threading
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import TsCamera

# COOPERATIVE TILES (csrc/raster.hip; ts_camera.hints bits 16..19): a forward compositing launch of at least COOP_FROM
# 16x16 tiles hands the COOP16 / 16 of every band that it dispatches last to workgroups of four waves.  Results do
# not depend on it (frame.py holds the frame path's copy of the two knobs).
COOP_FROM = int(os.environ.get("TS_HYBRID_FROM", "4096"))
COOP16 = max(0, min(15, int(os.environ.get("TS_HYBRID_COOP16", "3"))))

BLOCK = 16            # rasterize.py:19-20
CLIP_THRESH = 0.01    # gsplat's default near-plane threshold for project_gaussians


# --------------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------------
def num_sh_bases(degree: int) -> int:
    """Number of SH bases of a degree (call sites rasterize.py:76, model_gaussian.py:71)."""
    if degree == 0:
        return 1
    if degree == 1:
        return 4
    if degree == 2:
        return 9
    if degree == 3:
        return 16
    return 25


def deg_from_sh(num_bases: int) -> int:
    """Inverse of num_sh_bases (call site model_gaussian.py:106); raises on an invalid count."""
    for deg, nb in ((0, 1), (1, 4), (2, 9), (3, 16), (4, 25)):
        if nb == num_bases:
            return deg
    raise ValueError(f"Invalid number of SH bases: {num_bases}")


class _KernelTimer:
    """Optional per-entry timing with events recorded on the stream the kernels are launched on
    (torch's current stream).  Used by bench.py for the live roofline numbers; off by default.

    Entries that Python issues itself are bracketed by ``_call``; those of the native executors (csrc/frame.hip) by the
    library's entry probe, which calls ``_probe`` before and after each of them - a timed frame is the frame that runs."""

    def __init__(self):
        self.enabled = False
        self.records = {}
        self._open = {}         # thread -> event recorded when the executor entered the entry it is in (they do not nest)
        self._probe_c = _lib.ENTRY_PROBE(self._probe)       # (kept alive here: the library holds the bare pointer)

    def _probe(self, entry, end, _user):
        try:                    # called from native code: nothing may propagate
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if not end:
                self._open[threading.get_ident()] = ev
            else:
                self.records.setdefault(entry.decode(), []).append((self._open.pop(threading.get_ident()), ev))
        except Exception:
            pass

    def start(self):
        self.enabled = True
        self.records = {}
        self._open = {}
        _lib.load().ts_set_entry_probe(self._probe_c, None)

    def stop(self):
        """-> {entry: (launches, mean_ms)}; synchronises."""
        self.enabled = False
        _lib.load().ts_set_entry_probe(None, None)
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.records.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = (len(ms), sum(ms) / max(len(ms), 1))
        self.records = {}
        return out


kernel_timer = _KernelTimer()


def _call(name: str, fn, *args) -> None:
    """Invokes one C-ABI entry and raises on a non-zero status."""
    if kernel_timer.enabled:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        code = fn(*args)
        b.record()
        kernel_timer.records.setdefault(name, []).append((a, b))
    else:
        code = fn(*args)
    _lib.check(code, name)


def _need_hip(*tensors: Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if not isinstance(t, Tensor):
            raise TypeError("expected torch tensors")
        if not t.is_cuda:
            raise RuntimeError(
                "tinysplat_amd ops run only on a HIP (cuda) device; got a CPU tensor. "
                "There is deliberately no CPU fallback.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("all tensors must live on the same device")
    return dev


def _f32c(t: Tensor) -> Tensor:
    if t.dtype != torch.float32:
        raise ValueError(f"expected float32, got {t.dtype}")
    return t.contiguous()


def _i32c(t: Tensor) -> Tensor:
    if t.dtype != torch.int32:
        raise ValueError(f"expected int32, got {t.dtype}")
    return t.contiguous()


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev: torch.device) -> int:
    """raw handle of torch's current stream on ``dev`` (torch.cuda.current_stream() builds a Stream object: ~10 us of a
    small scene's 280 us of host time per step, three times per step - round 6, tools/host_cprofile.py)"""
    if _raw_stream is not None and dev.index is not None:
        return int(_raw_stream(dev.index))
    return torch.cuda.current_stream(dev).cuda_stream


def _camera(fx, fy, cx, cy, img_height, img_width, tile_bounds, glob_scale=1.0,
            clip_thresh=CLIP_THRESH, tile_rows: Optional[Tuple[int, int]] = None,
            wide_tiles: bool = False) -> TsCamera:
    tbx, tby = int(tile_bounds[0]), int(tile_bounds[1])
    if tile_rows is None:
        row0, rows = 0, tby
    else:
        row0, rows = int(tile_rows[0]), int(tile_rows[1]) - int(tile_rows[0])
        if row0 < 0 or rows < 0 or row0 + rows > tby:
            raise ValueError(f"tile_rows {tile_rows} outside [0, {tby}]")
    return TsCamera(float(fx), float(fy), float(cx), float(cy), int(img_width), int(img_height),
                    tbx, tby, row0, rows, float(glob_scale), float(clip_thresh), 1 if wide_tiles else 0, 0)


def _tile_bounds(img_height: int, img_width: int) -> Tuple[int, int, int]:
    return ((img_width + BLOCK - 1) // BLOCK, (img_height + BLOCK - 1) // BLOCK, 1)


# --------------------------------------------------------------------------------------------------
# project_gaussians
# --------------------------------------------------------------------------------------------------
class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
                img_height, img_width, tile_bounds, clip_thresh, tile_rows, flags):
        dev = _need_hip(means3d, scales, quats, viewmat, projmat)
        n = means3d.shape[0]
        if means3d.shape != (n, 3) or scales.shape != (n, 3) or quats.shape != (n, 4):
            raise ValueError("means3d [N,3], scales [N,3], quats [N,4] expected")
        if viewmat.numel() < 12 or projmat.shape != (4, 4):
            raise ValueError("viewmat must hold the 3x4 view rows, projmat must be [4,4]")
        means3d, scales, quats = _f32c(means3d), _f32c(scales), _f32c(quats)
        viewmat, projmat = _f32c(viewmat), _f32c(projmat)
        cam = _camera(fx, fy, cx, cy, img_height, img_width, tile_bounds, glob_scale, clip_thresh,
                      tile_rows)
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        xys = torch.empty((n, 2), **f32)
        depths = torch.empty((n,), **f32)
        radii = torch.empty((n,), **i32)
        conics = torch.empty((n, 3), **f32)
        nth = torch.empty((n,), **i32)
        cov3d = torch.empty((n, 6), **f32)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_project_fwd", lib.ts_project_fwd, n, _ptr(means3d), _ptr(scales), _ptr(quats), _ptr(viewmat),
                                          _ptr(projmat), cam, int(flags), _ptr(xys), _ptr(depths), _ptr(radii),
                                          _ptr(conics), _ptr(nth), _ptr(cov3d), _stream(dev))
        ctx.cam, ctx.flags = cam, int(flags)
        ctx.save_for_backward(means3d, scales, quats, viewmat, projmat, radii)
        ctx.mark_non_differentiable(radii, nth)
        ctx.set_materialize_grads(False)
        return xys, depths, radii, conics, nth, cov3d

    @staticmethod
    def backward(ctx, v_xys, v_depths, _v_radii, v_conics, _v_nth, v_cov3d):
        means3d, scales, quats, viewmat, projmat, radii = ctx.saved_tensors
        dev = means3d.device
        n = means3d.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        v_xys = torch.zeros((n, 2), **f32) if v_xys is None else _f32c(v_xys)
        v_depths = torch.zeros((n,), **f32) if v_depths is None else _f32c(v_depths)
        v_conics = torch.zeros((n, 3), **f32) if v_conics is None else _f32c(v_conics)
        v_cov3d = None if v_cov3d is None else _f32c(v_cov3d)
        v_means = torch.empty((n, 3), **f32)
        v_scales = torch.empty((n, 3), **f32)
        v_quats = torch.empty((n, 4), **f32)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_project_bwd", lib.ts_project_bwd, n, _ptr(means3d), _ptr(scales), _ptr(quats), _ptr(viewmat),
                                          _ptr(projmat), ctx.cam, ctx.flags, _ptr(radii), _ptr(v_xys),
                                          _ptr(v_depths), _ptr(v_conics), _ptr(v_cov3d),
                                          _ptr(v_means), _ptr(v_scales), _ptr(v_quats),
                                          _stream(dev))
        return (v_means, v_scales, None, v_quats) + (None,) * 12


def project_gaussians(means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor,
                      viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
                      img_height: int, img_width: int, tile_bounds: Tuple[int, int, int],
                      clip_thresh: float = CLIP_THRESH,
                      tile_rows: Optional[Tuple[int, int]] = None, log_scales: bool = False,
                      raw_quats: bool = False):
    """EWA projection of N Gaussians.  Same positional signature tinysplat calls at rasterize.py:32.

    Returns ``(xys[N,2], depths[N], radii[N] int32, conics[N,3], num_tiles_hit[N] int32,
    cov3d[N,6])``; differentiable w.r.t. ``means3d``, ``scales``, ``quats``.  ``tile_rows=(r0,r1)``
    (extension, multi-GPU stripes) restricts ``num_tiles_hit`` to tile rows [r0, r1).
    ``log_scales`` / ``raw_quats`` (extensions) fold the adapter's ``exp(scales)`` and
    ``quats / |quats|`` (rasterize.py:72-73) into the kernel; gradients are then w.r.t. the raw
    tensors.
    """
    flags = (1 if log_scales else 0) | (2 if raw_quats else 0)
    return _ProjectGaussians.apply(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx,
                                   cy, img_height, img_width, tile_bounds, clip_thresh, tile_rows,
                                   flags)


# --------------------------------------------------------------------------------------------------
# opacity compensation of the antialiased mode (csrc/antialias.hip)
# --------------------------------------------------------------------------------------------------
RASTERIZE_MODES = ("classic", "antialiased")


def rasterize_mode(model) -> str:
    """``model.rasterize_mode``, "classic" for a model without the attribute; anything else raises."""
    mode = getattr(model, "rasterize_mode", "classic")
    if mode not in RASTERIZE_MODES:
        raise ValueError(f"rasterize_mode {mode!r}: expected one of {RASTERIZE_MODES}")
    return mode


def refuse_antialiased(model, what: str) -> None:
    """Raises for an antialiased model on a path the mode is not built for (the sharded trainers)."""
    if rasterize_mode(model) == "antialiased":
        raise NotImplementedError(f"{what} does not render rasterize_mode 'antialiased' (DESIGN.md section 6w: the sharded "
                                  "paths are out of scope): render on one GPU, or use the classic mode")


class _OpacityCompensation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, img_height, img_width, clip_thresh,
                flags):
        dev = _need_hip(means3d, scales, quats, viewmat)
        n = means3d.shape[0]
        if means3d.shape != (n, 3) or scales.shape != (n, 3) or quats.shape != (n, 4):
            raise ValueError("means3d [N,3], scales [N,3], quats [N,4] expected")
        if viewmat.numel() < 12:
            raise ValueError("viewmat must hold the 3x4 view rows")
        means3d, scales, quats, viewmat = _f32c(means3d), _f32c(scales), _f32c(quats), _f32c(viewmat)
        cam = _camera(fx, fy, cx, cy, img_height, img_width, _tile_bounds(img_height, img_width), glob_scale, clip_thresh)
        comp = torch.empty((n,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _call("ts_antialias_fwd", _lib.load().ts_antialias_fwd, n, _ptr(means3d), _ptr(scales), _ptr(quats),
                  _ptr(viewmat), cam, int(flags), None, 0, _ptr(comp), None, None, _stream(dev))
        ctx.cam, ctx.flags = cam, int(flags)
        ctx.save_for_backward(means3d, scales, quats, viewmat)
        return comp

    @staticmethod
    def backward(ctx, v_comp):
        means3d, scales, quats, viewmat = ctx.saved_tensors
        dev = means3d.device
        n = means3d.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        v_comp = _f32c(v_comp)
        v_means, v_scales, v_quats = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32), torch.empty((n, 4), **f32)
        with torch.cuda.device(dev):
            _call("ts_compensation_bwd", _lib.load().ts_compensation_bwd, n, _ptr(means3d), _ptr(scales), _ptr(quats),
                  _ptr(viewmat), ctx.cam, ctx.flags, _ptr(v_comp), _ptr(v_means), _ptr(v_scales), _ptr(v_quats),
                  _stream(dev))
        return (v_means, v_scales, None, v_quats) + (None,) * 9


def opacity_compensation(means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor, viewmat: Tensor,
                         fx: float, fy: float, cx: float, cy: float, img_height: int, img_width: int,
                         clip_thresh: float = CLIP_THRESH, log_scales: bool = False, raw_quats: bool = False) -> Tensor:
    """``comp[N] = sqrt(max(0, det(cov2d) / det(cov2d + 0.3 I)))`` of the covariance ``project_gaussians`` projects, before
    its blur: the factor the antialiased mode scales an opacity by (0 behind the clip plane and where the max clamps,
    with a zero gradient there).  Differentiable w.r.t. ``means3d``, ``scales``, ``quats``; ``log_scales`` /
    ``raw_quats`` as in ``project_gaussians``."""
    flags = (1 if log_scales else 0) | (2 if raw_quats else 0)
    return _OpacityCompensation.apply(means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, img_height, img_width,
                                      clip_thresh, flags)


def compensated_opacity(model, viewmat: Tensor, fx: float, fy: float, width: int, height: int, op=None) -> Tensor:
    """``sigmoid(model.opacities) * comp`` in the shape of ``model.opacities``: the plain opacity an op-by-op consumer of
    an antialiased model hands to ``rasterize_gaussians`` (without ``logit_opacity``) in place of the logits.  ``op``: the
    compensation op of a pluggable ops namespace (``GaussianRasterizer.ops``); None: ``opacity_compensation``."""
    comp = (op or opacity_compensation)(model.means, model.scales, 1., model.quats, viewmat, fx, fy, width / 2, height / 2,
                                        height, width, log_scales=True, raw_quats=True)
    return torch.sigmoid(model.opacities) * comp.view(model.opacities.shape)


# --------------------------------------------------------------------------------------------------
# spherical_harmonics
# --------------------------------------------------------------------------------------------------
class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degrees_to_use, viewdirs, coeffs):
        dev = _need_hip(viewdirs, coeffs)
        if coeffs.dim() != 3 or coeffs.shape[-1] != 3:
            raise ValueError("coeffs must be [N, K, 3]")
        n, nb = coeffs.shape[0], coeffs.shape[1]
        if viewdirs.shape != (n, 3):
            raise ValueError("viewdirs must be [N, 3]")
        stored = deg_from_sh(nb)
        if degrees_to_use < 0 or degrees_to_use > stored:
            raise ValueError(f"degrees_to_use={degrees_to_use} not in [0, {stored}]")
        viewdirs, coeffs = _f32c(viewdirs), _f32c(coeffs)
        colors = torch.empty((n, 3), dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_sh_fwd", lib.ts_sh_fwd, n, int(degrees_to_use), nb, _ptr(viewdirs), _ptr(coeffs),
                                     _ptr(colors), _stream(dev))
        ctx.degree, ctx.nb = int(degrees_to_use), nb
        ctx.save_for_backward(viewdirs)
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        (viewdirs,) = ctx.saved_tensors
        dev = viewdirs.device
        n = viewdirs.shape[0]
        v_colors = _f32c(v_colors)
        v_coeffs = torch.empty((n, ctx.nb, 3), dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_sh_bwd", lib.ts_sh_bwd, n, ctx.degree, ctx.nb, _ptr(viewdirs), _ptr(v_colors),
                                     _ptr(v_coeffs), _stream(dev))
        return None, None, v_coeffs


def spherical_harmonics(degrees_to_use: int, viewdirs: Tensor, coeffs: Tensor) -> Tensor:
    """colors[N,3] from SH coefficients [N,K,3]; signature of the call at rasterize.py:38.
    Differentiable w.r.t. ``coeffs`` only (no gradient to ``viewdirs``, as upstream)."""
    return _SphericalHarmonics.apply(degrees_to_use, viewdirs, coeffs)


class _ShColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degrees_to_use, means3d, origin, colors_dc, colors_rest):
        dev = _need_hip(means3d, origin, colors_dc, colors_rest)
        n = means3d.shape[0]
        if means3d.shape != (n, 3) or colors_dc.shape != (n, 3) or origin.numel() != 3:
            raise ValueError("means3d [N,3], origin [3], colors_dc [N,3] expected")
        if colors_rest.dim() != 3 or colors_rest.shape[0] != n or colors_rest.shape[2] != 3:
            raise ValueError("colors_rest must be [N, K-1, 3]")
        nb = colors_rest.shape[1] + 1
        stored = deg_from_sh(nb)
        if degrees_to_use < 0 or degrees_to_use > stored:
            raise ValueError(f"degrees_to_use={degrees_to_use} not in [0, {stored}]")
        means3d, origin = _f32c(means3d), _f32c(origin)
        colors_dc, colors_rest = _f32c(colors_dc), _f32c(colors_rest)
        colors = torch.empty((n, 3), dtype=torch.float32, device=dev)
        mask = torch.empty((n,), dtype=torch.uint8, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_sh_colors_fwd", lib.ts_sh_colors_fwd, n, int(degrees_to_use), nb, _ptr(means3d),
                  _ptr(origin), _ptr(colors_dc), _ptr(colors_rest) if nb > 1 else None, _ptr(colors),
                  _ptr(mask), None, _stream(dev))
        ctx.degree, ctx.nb = int(degrees_to_use), nb
        ctx.save_for_backward(means3d, origin, mask)
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        means3d, origin, mask = ctx.saved_tensors
        dev = means3d.device
        n = means3d.shape[0]
        v_colors = _f32c(v_colors)
        v_dc = torch.empty((n, 3), dtype=torch.float32, device=dev)
        v_rest = torch.empty((n, ctx.nb - 1, 3), dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _call("ts_sh_colors_bwd", lib.ts_sh_colors_bwd, n, ctx.degree, ctx.nb, _ptr(means3d),
                  _ptr(origin), _ptr(mask), _ptr(v_colors), _ptr(v_dc),
                  _ptr(v_rest) if ctx.nb > 1 else None, _stream(dev))
        return None, None, None, v_dc, v_rest


def sh_colors(degrees_to_use: int, means3d: Tensor, origin: Tensor, colors_dc: Tensor,
              colors_rest: Tensor) -> Tensor:
    """Fused colour stage of the render adapter: what rasterize.py:75-81 + :38-39 compute
    (``clamp(spherical_harmonics(deg, normalize(means - origin), cat(dc, rest)) + 0.5, min=0)``)
    without materialising the view directions or the 192 N-byte ``torch.cat``.  Differentiable
    w.r.t. ``colors_dc`` and ``colors_rest`` (no gradient to ``means3d``, as in the reference where
    the SH op returns none for the view directions)."""
    return _ShColors.apply(degrees_to_use, means3d, origin, colors_dc, colors_rest)


# --------------------------------------------------------------------------------------------------
# rasterize_gaussians
# --------------------------------------------------------------------------------------------------
class TileBinning:
    """Result of the binning stages: everything compositing needs besides colours."""
    __slots__ = ("cam", "n", "num_tiles", "num_intersects", "cum_tiles_hit", "tile_bins",
                 "gaussian_ids_sorted", "num_tiles_hit", "_keep", "_versions")


_bin_cache = {}


def _same(t: Tensor, kept: Tensor, version: int) -> bool:
    return (t.data_ptr() == kept.data_ptr() and t._version == version and t.shape == kept.shape)


_pinned_counts = {}


class _IntersectionCount:
    """The path's one host read - cum_tiles_hit[n-1], which sizes the intersection buffers - as an
    asynchronous copy into pinned memory plus an event: the caller keeps enqueueing the kernels
    that do not depend on the count and waits only when it must allocate."""

    def __init__(self, cum: Tensor, dev: torch.device):
        self.n = cum.shape[0]
        if self.n == 0:
            return
        slot = _pinned_counts.get(dev.index)
        if slot is None:
            slot = (torch.empty((1,), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
            _pinned_counts[dev.index] = slot
        self.host, self.event = slot
        self.host.copy_(cum[-1:], non_blocking=True)
        self.event.record(torch.cuda.current_stream(dev))

    def wait(self) -> int:
        if self.n == 0:
            return 0
        self.event.synchronize()
        total = int(self.host[0])
        if total < 0:
            raise OverflowError("more than 2^31-1 tile intersections: num_tiles_hit overflows its "
                                "int32 prefix sum (gsplat's cum_tiles_hit is int32 as well)")
        return total


def bin_gaussians(xys: Tensor, depths: Tensor, radii: Tensor, num_tiles_hit: Tensor,
                  img_height: int, img_width: int,
                  tile_rows: Optional[Tuple[int, int]] = None, use_cache: bool = True) -> TileBinning:
    """cumsum -> per-tile count -> offsets -> scatter -> per-tile depth sort.

    tinysplat rasterizes twice per frame on identical (xys, depths, radii, num_tiles_hit)
    (rasterize.py:44 and :50); the result is memoised on the identity (storage address + version
    counter) of those tensors, whose storages are kept alive by the cache entry, so the second call
    and the backward reuse it.
    """
    dev = _need_hip(xys, depths, radii, num_tiles_hit)
    n = xys.shape[0]
    xys_c, depths_c = _f32c(xys.detach()), _f32c(depths.detach())
    radii_c, nth_c = _i32c(radii), _i32c(num_tiles_hit)
    tb = _tile_bounds(img_height, img_width)
    cam = _camera(0.0, 0.0, 0.0, 0.0, img_height, img_width, tb, tile_rows=tile_rows)
    if cam.tile_rows * cam.tile_bounds_x >= COOP_FROM:      # COOPERATIVE TILES of the forward launch (a pure hint)
        cam.hints |= COOP16 << 16
    key = (dev.index, int(img_height), int(img_width), cam.tile_row0, cam.tile_rows)
    if use_cache:
        hit = _bin_cache.get(dev.index)
        if hit is not None and hit[0] == key:
            b = hit[1]
            if all(_same(t, k, v) for t, k, v in zip((xys_c, depths_c, radii_c, nth_c), b._keep,
                                                     b._versions)):
                return b
    lib = _lib.load()
    s = _stream(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    num_tiles = cam.tile_rows * cam.tile_bounds_x
    b = TileBinning()
    b.cam, b.n, b.num_tiles, b.num_tiles_hit = cam, n, num_tiles, nth_c
    with torch.cuda.device(dev):
        cum = torch.empty((n,), **i32)
        ws = torch.empty((int(lib.ts_scan_ws_ints(n)),), **i32)
        _call("ts_scan_tiles", lib.ts_scan_tiles, n, _ptr(nth_c), _ptr(cum), _ptr(ws), None, s)
        pending = _IntersectionCount(cum, dev)       # D2H copy of cum[n-1] starts now ...
        bin_ws = torch.empty((int(lib.ts_bin_ws_ints(n, num_tiles)),), **i32)
        tile_bins = torch.empty((max(num_tiles, 1), 2), **i32)
        _call("ts_bin_count", lib.ts_bin_count, n, _ptr(xys_c), _ptr(radii_c), None, cam, _ptr(bin_ws), s)
        _call("ts_tile_offsets", lib.ts_tile_offsets, n, num_tiles, _ptr(bin_ws), _ptr(tile_bins), None, -1, s)
        total = pending.wait()                       # ... and is awaited behind the two launches above
        bucket_ids = torch.empty((max(total, 1),), **i32)
        ids = torch.empty((max(total, 1),), **i32)
        if total > 0:
            _call("ts_bin_scatter", lib.ts_bin_scatter, n, _ptr(xys_c), _ptr(radii_c), None, cam,
                  _ptr(bin_ws), _ptr(bucket_ids), _ptr(ids), s)
            _call("ts_sort_tiles", lib.ts_sort_tiles, num_tiles, _ptr(tile_bins), _ptr(depths_c),
                  _ptr(bucket_ids), _ptr(ids), _ptr(bin_ws), bin_ws.data_ptr() + 4 * (bin_ws.numel() - 1), s)
    b.num_intersects = total
    b.cum_tiles_hit = cum
    b.tile_bins = tile_bins[:num_tiles]
    b.gaussian_ids_sorted = ids[:total]
    b._keep = (xys_c, depths_c, radii_c, nth_c)
    b._versions = tuple(t._version for t in b._keep)
    if use_cache:
        _bin_cache[dev.index] = (key, b)
    return b


def clear_binning_cache() -> None:
    _bin_cache.clear()


def _stripe_rows(cam: TsCamera) -> int:
    return max(0, min(BLOCK * cam.tile_rows, cam.img_height - BLOCK * cam.tile_row0))


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height,
                img_width, background, tile_rows, logit_opacity):
        dev = _need_hip(xys, depths, radii, conics, num_tiles_hit, colors, opacity, background)
        n = xys.shape[0]
        if colors.dim() != 2 or colors.shape[0] != n or colors.shape[1] not in (3, 4):
            raise ValueError("colors must be [N,3] (or [N,4])")
        ch = colors.shape[1]
        if xys.shape != (n, 2) or conics.shape != (n, 3) or opacity.numel() != n:
            raise ValueError("xys [N,2], conics [N,3], opacity [N,1] expected")
        if background.numel() != ch:
            raise ValueError(f"background must have {ch} entries")
        b = bin_gaussians(xys, depths, radii, num_tiles_hit, img_height, img_width, tile_rows)
        cam = b.cam
        xys_c, conics_c = _f32c(xys), _f32c(conics)
        colors_c, opac_c, bg_c = _f32c(colors), _f32c(opacity), _f32c(background)
        rows = _stripe_rows(cam)
        W = int(img_width)
        f32 = dict(dtype=torch.float32, device=dev)
        splats = torch.empty((max(n, 1), 12), **f32)
        out_img = torch.empty((rows, W, ch), **f32)
        final_Ts = torch.empty((rows, W), **f32)
        final_idx = torch.empty((rows, W), dtype=torch.int32, device=dev)
        lib = _lib.load()
        s = _stream(dev)
        with torch.cuda.device(dev):
            _call("ts_pack_splats", lib.ts_pack_splats, n, ch, 1 if logit_opacity else 0, _ptr(xys_c), _ptr(b._keep[2]), _ptr(conics_c),
                                          _ptr(colors_c), _ptr(opac_c), _ptr(b.cum_tiles_hit), cam,
                                          None, _ptr(splats), s)
            _call("ts_raster_fwd", lib.ts_raster_fwd, ch, 0, cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted),
                                         _ptr(splats), _ptr(bg_c), _ptr(out_img), _ptr(final_Ts),
                                         _ptr(final_idx), None, s)
        out_alpha = 1.0 - final_Ts
        ctx.binning, ctx.ch, ctx.n = b, ch, n
        ctx.logit = 1 if logit_opacity else 0
        ctx.opacity_shape = opacity.shape
        ctx.save_for_backward(splats, bg_c, final_Ts, final_idx)
        ctx.set_materialize_grads(False)
        return out_img, out_alpha

    @staticmethod
    def backward(ctx, v_out_img, v_out_alpha):
        splats, bg_c, final_Ts, final_idx = ctx.saved_tensors
        b, ch, n = ctx.binning, ctx.ch, ctx.n
        dev = splats.device
        f32 = dict(dtype=torch.float32, device=dev)
        if v_out_img is None:
            v_out_img = torch.zeros(final_Ts.shape + (ch,), **f32)
        v_out_img = _f32c(v_out_img)
        v_out_alpha = None if v_out_alpha is None else _f32c(v_out_alpha)
        total = b.num_intersects
        # the four 2-D gradients are views of ONE allocation, in this order, so that the multi-GPU
        # path can all-reduce them in place as a single buffer (sharding._SumGradsAcrossRanks)
        flat = torch.empty((n * (6 + ch),), **f32)
        v_xy = flat[:2 * n].view(n, 2)
        v_conic = flat[2 * n:5 * n].view(n, 3)
        v_colors = flat[5 * n:(5 + ch) * n].view(n, ch)
        v_opacity = flat[(5 + ch) * n:]
        partials = torch.empty((max(total, 1), _lib.PARTIAL_ROW_FLOATS), **f32)
        row_flags = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
        lib = _lib.load()
        s = _stream(dev)
        with torch.cuda.device(dev):
            _call("ts_raster_bwd", lib.ts_raster_bwd, ch, 0, total, b.cam, _ptr(b.tile_bins),
                                         _ptr(b.gaussian_ids_sorted), _ptr(splats), _ptr(bg_c),
                                         _ptr(final_Ts), _ptr(final_idx), _ptr(v_out_img),
                                         _ptr(v_out_alpha), None, _ptr(partials), _ptr(row_flags), s)
            _call("ts_reduce_partials", lib.ts_reduce_partials, n, ch, ctx.logit, _ptr(b.num_tiles_hit), _ptr(b.cum_tiles_hit),
                                              _ptr(partials), _ptr(row_flags), _ptr(splats), _ptr(v_xy), _ptr(v_conic),
                                              _ptr(v_colors), _ptr(v_opacity), None, None, s)
        return (v_xy, None, None, v_conic, None, v_colors, v_opacity.view(ctx.opacity_shape),
                None, None, None, None, None)


def rasterize_gaussians(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor,
                        num_tiles_hit: Tensor, colors: Tensor, opacity: Tensor, img_height: int,
                        img_width: int, background: Tensor,
                        tile_rows: Optional[Tuple[int, int]] = None, logit_opacity: bool = False):
    """Tile-based alpha compositing; positional signature of the calls at rasterize.py:44,50.

    Returns the 2-tuple ``(out_img[H,W,C], out_alpha[H,W])`` that tinysplat unpacks
    (``rgbs, _ = rasterize_gaussians(*inputs)``).  Differentiable w.r.t. ``xys``, ``conics``,
    ``colors``, ``opacity``.  With ``tile_rows=(r0,r1)`` only that stripe of tile rows is rendered
    and the outputs hold its pixel rows.  ``logit_opacity=True`` (extension) takes opacity logits and
    folds the adapter's ``sigmoid`` (rasterize.py:86) into the kernels.
    """
    return _RasterizeGaussians.apply(xys, depths, radii, conics, num_tiles_hit, colors, opacity,
                                     img_height, img_width, background, tile_rows, logit_opacity)
