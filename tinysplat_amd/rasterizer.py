"""Render adapter: the build's counterpart of tinysplat's ``GaussianRasterizer``.

Mirrors /root/reference/tinysplat/splatting/rasterize.py:13-94 - same constructor, same
``__call__(camera, dims, sh_degree) -> (rgb[H,W,3], extras)`` contract, same argument lists handed
to the three ops (so a model/camera pair produces bit-identical boundary traffic), same frame
recipe: project -> retain xys grad -> SH -> clamp(rgb+0.5, min 0) -> rasterize RGB -> clamp(max 1)
-> rasterize depth replicated to 3 channels -> depth = channel 0.

Two reference quirks are reproduced on purpose (results parity with tinysplat):
  * SH view directions are ``means - view_matrix[:3,3]`` (the translation column, rasterize.py:77),
    not ``means - camera_position`` (``correct_viewdirs=True`` switches to the camera centre: SURVEY App. C #9);
  * the depth image is composited with ``model.background`` (rasterize.py:86), so it contains
    ``T_final * background[0]``.
The ``sh_degree`` argument is accepted and ignored, as in the reference (model.active_sh_degree is
used, rasterize.py:81).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional, Sequence, Tuple

import torch

from . import frame as _hip_frame
from . import ops as _hip_ops

TILE = 16  # rasterize.py:19-20


def tile_bounds(dims: Tuple[int, int]) -> Tuple[int, int, int]:
    """(ceil(W/16), ceil(H/16), 1) for dims = (W, H); rasterize.py:88-94."""
    w, h = int(dims[0]), int(dims[1])
    return (-(-w // TILE), -(-h // TILE), 1)


_cam_cache = {}


def sh_origin(view_matrix, correct_viewdirs: bool = False):
    """The point the SH view directions are taken from.  Reference (rasterize.py:77): ``view_matrix[:3, 3]`` - the
    TRANSLATION column of the world-to-camera transform, not the camera; ``correct_viewdirs``: the
    camera centre ``-R^T t`` (= ``inv(view_matrix)[:3, 3]``, the `position` of scene.py:96-107)."""
    t = view_matrix[:3, 3]
    if not correct_viewdirs:
        return t.contiguous()
    return (-(view_matrix[:3, :3].T @ t)).contiguous()


def camera_on_device(camera, device, correct_viewdirs: bool = False):
    """(view[4,4], proj @ view [4,4], origin[3]) on `device`, memoised on the identity/version of the
    camera's two matrices: the reference re-uploads them every frame (rasterize.py:70-71), which on
    a GPU is two pageable host->device copies and a 4x4 GEMM launch per frame."""
    vm, pm = camera.view_matrix, camera.proj_matrix
    key = (id(camera), str(device), bool(correct_viewdirs))
    sig = (vm.data_ptr(), vm._version, pm.data_ptr(), pm._version)
    hit = _cam_cache.get(key)
    if hit is not None and hit[0] == sig:
        return hit[1]
    view = vm.to(device)
    out = (view, pm.to(device) @ view, sh_origin(vm, correct_viewdirs).to(device))
    if len(_cam_cache) > 64:
        _cam_cache.clear()
    _cam_cache[key] = (sig, out, vm, pm)     # keep the tensors alive so data_ptr stays unique
    return out


def project_args(model, camera, dims, device):
    """The 13 positional arguments of project_gaussians (rasterize.py:64-73)."""
    w, h = dims
    view = camera.view_matrix.to(device)
    proj = camera.proj_matrix.to(device)
    unit_quats = model.quats / model.quats.norm(dim=-1, keepdim=True)
    return [model.means, torch.exp(model.scales), 1., unit_quats, view[:3, :], proj @ view,
            camera.f_x, camera.f_y, w / 2, h / 2, h, w, tile_bounds(dims)]


def sh_args(model, camera, device, correct_viewdirs: bool = False):
    """[active degree, view directions, coefficients[N,K,3]] (rasterize.py:75-81)."""
    origin = sh_origin(camera.view_matrix, correct_viewdirs).to(device)     # reference quirk: translation column
    dirs = model.means - origin
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    coeffs = torch.cat([model.colors_dc[:, None, :], model.colors_rest], dim=1)
    return [model.active_sh_degree, dirs, coeffs]


def raster_args(model, xys, depths, radii, conics, num_tiles, colors, dims):
    """The 10 positional arguments of rasterize_gaussians (rasterize.py:83-86)."""
    w, h = dims
    return [xys, depths, radii, conics, num_tiles, colors, torch.sigmoid(model.opacities), h, w,
            model.background]


class GaussianRasterizer:
    BLOCK_X = TILE
    BLOCK_Y = TILE

    def __init__(self, model, cameras: Optional[Sequence] = None, device=torch.device("cuda:0"),
                 fused_colors: bool = True, correct_viewdirs: bool = False):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.model = model
        self.global_scale = torch.tensor([1.0])
        # the reference takes the SH view directions from the view matrix's translation column
        # (rasterize.py:77), which is the camera position only for an unrotated camera; True = from the camera centre
        # (what gsplat's own examples feed the op).  Default: the reference's results.
        self.correct_viewdirs = bool(correct_viewdirs)
        # fused_colors: compute rasterize.py:75-81 + :38-39 (view dirs, cat, SH, +0.5, clamp) in one
        # HIP kernel when the ops namespace offers it; False = the reference's op-by-op recipe.
        # fused_prep: likewise fold exp(scales), quats/|quats| (rasterize.py:72-73) and
        # sigmoid(opacities) (rasterize.py:86) into the projection / packing kernels.
        # fused_depth: composite RGB and depth in ONE 4-channel pass (the kernels are templated on
        # the channel count) instead of two 3-channel passes over the same lists.
        # single_node: run all of it as one autograd function (frame.py) to cut host overhead.
        self.fused_colors = fused_colors
        self.fused_prep = fused_colors
        self.fused_depth = fused_colors
        self.single_node = fused_colors
        # the three callables of the boundary; the product default is the HIP library
        self.ops = SimpleNamespace(project_gaussians=_hip_ops.project_gaussians,
                                   spherical_harmonics=_hip_ops.spherical_harmonics,
                                   rasterize_gaussians=_hip_ops.rasterize_gaussians,
                                   sh_colors=_hip_ops.sh_colors, fused_prep=True,
                                   four_channels=True, render_frame=_hip_frame.render_frame,
                                   render_view=_hip_frame.render_view,
                                   render_frame_planes=_hip_frame.render_frame_planes,
                                   opacity_compensation=_hip_ops.opacity_compensation)

    def __call__(self, camera, dims=None, sh_degree: Optional[int] = None):
        if dims is None:
            dims = (camera.width, camera.height)
        ops = self.ops

        prep = self.fused_prep and getattr(ops, "fused_prep", False)
        if (prep and self.fused_colors and self.fused_depth and self.single_node
                and getattr(ops, "render_frame", None) is not None):
            # everything above in one autograd node (frame.py): same kernels, a fraction of the
            # host-side cost per frame
            view, projview, origin = camera_on_device(camera, self.device, self.correct_viewdirs)
            w, h = dims
            # under torch.no_grad() (the viewer, viewer.py:89-93) nothing is kept for backward
            planes = getattr(ops, "render_frame_planes", None)
            if planes is not None:
                # rgb and depth as two contiguous images (what rasterize.py:45 and :51 hand out), composited in
                # one 4-channel pass: nothing downstream slices an interleaved image, forward or backward
                if torch.is_grad_enabled():
                    rgb, depth, xys, radii = planes(self.model, view[:3, :], projview, origin, camera.f_x,
                                                    camera.f_y, w, h)
                else:
                    rgb, depth, xys, radii = ops.render_view(self.model, view[:3, :], projview, origin,
                                                             camera.f_x, camera.f_y, w, h, True, planes=True)
            else:
                # under torch.no_grad() (the viewer, viewer.py:89-93) nothing is kept for backward
                fn = ops.render_frame if torch.is_grad_enabled() else getattr(ops, "render_view", ops.render_frame)
                out, xys, radii = fn(self.model, view[:3, :], projview, origin, camera.f_x, camera.f_y,
                                     w, h, True)
                rgb, depth = out[:, :, :3], out[:, :, 3]
            extras = {"depth": depth, "radii": radii, "xys": xys,
                      "camera": {"height": camera.height, "width": camera.width}}
            return rgb, extras                     # clamp(max=1) is applied inside the kernels
        if prep:
            w, h = dims
            _, projview, _ = camera_on_device(camera, self.device)
            view = camera_on_device(camera, self.device)[0]
            model = self.model
            xys, depths, radii, conics, num_tiles, _cov3d = ops.project_gaussians(
                model.means, model.scales, 1., model.quats, view[:3, :], projview, camera.f_x,
                camera.f_y, w / 2, h / 2, h, w, tile_bounds(dims), log_scales=True, raw_quats=True)
            rkw = {"logit_opacity": True}
        else:
            xys, depths, radii, conics, num_tiles, _cov3d = ops.project_gaussians(
                *self.project_forward_inputs(camera, dims))
            rkw = {}
        if xys.requires_grad:
            xys.retain_grad()          # model_gaussian.py:130-132 reads extras['xys'].grad

        colors = self.colors(camera)
        o_eff = self._compensated_opacity(camera, dims)
        if o_eff is not None:              # antialiased model: a plain opacity takes the place of the logits / the sigmoid
            rkw = {}

        if self.fused_depth and getattr(ops, "four_channels", False):
            # one 4-channel compositing pass instead of the reference's two 3-channel ones
            # (rasterize.py:44 and :50): channel 3 carries the depth, its background is
            # background[0] exactly as in the reference's depth pass (rasterize.py:86)
            ra = self._raster_inputs(xys, depths, radii, conics, num_tiles,
                                     torch.cat([colors, depths[:, None]], dim=1), dims, prep, o_eff)
            ra[9] = torch.cat([ra[9], ra[9][:1]])
            out, _ = ops.rasterize_gaussians(*ra, **rkw)
            rgb = torch.clamp(out[:, :, :3], max=1.0)
            depth_map = out[:, :, 3]
        else:
            rgb, _ = ops.rasterize_gaussians(*self._raster_inputs(
                xys, depths, radii, conics, num_tiles, colors, dims, prep, o_eff), **rkw)
            rgb = torch.clamp(rgb, max=1.0)
            depth_as_color = depths[:, None].repeat(1, 3)
            depth_img, _ = ops.rasterize_gaussians(*self._raster_inputs(
                xys, depths, radii, conics, num_tiles, depth_as_color, dims, prep, o_eff), **rkw)
            depth_map = depth_img[:, :, 0]

        extras = {"depth": depth_map, "radii": radii, "xys": xys,
                  "camera": {"height": camera.height, "width": camera.width}}
        return rgb, extras

    def _raster_inputs(self, xys, depths, radii, conics, num_tiles, colors, dims, prep, o_eff=None):
        w, h = dims
        if o_eff is not None:
            return [xys, depths, radii, conics, num_tiles, colors, o_eff, h, w, self.model.background]
        if not prep:
            return self.rasterize_forward_inputs(xys, depths, radii, conics, num_tiles, colors, dims)
        return [xys, depths, radii, conics, num_tiles, colors, self.model.opacities, h, w,
                self.model.background]

    def _compensated_opacity(self, camera, dims):
        """The op-by-op paths of an antialiased model: ``sigmoid(opacities) * comp`` from the
        compensation op of the ops namespace, handed to rasterize_gaussians as a plain opacity; None for a classic model."""
        if _hip_ops.rasterize_mode(self.model) != "antialiased":
            return None
        op = getattr(self.ops, "opacity_compensation", None)
        if op is None:
            raise RuntimeError("rasterize_mode 'antialiased' needs an ops namespace with opacity_compensation")
        w, h = dims
        view = camera_on_device(camera, self.device)[0]
        return _hip_ops.compensated_opacity(self.model, view[:3, :], camera.f_x, camera.f_y, w, h, op=op)

    def colors(self, camera):
        """Per-Gaussian RGB handed to the rasterizer: clamp(SH(...) + 0.5, min=0)."""
        fused = getattr(self.ops, "sh_colors", None) if self.fused_colors else None
        if fused is not None:
            m = self.model
            origin = camera_on_device(camera, self.device, self.correct_viewdirs)[2]
            return fused(m.active_sh_degree, m.means, origin, m.colors_dc, m.colors_rest)
        colors = self.ops.spherical_harmonics(*self.spherical_harmonics_inputs(camera))
        return torch.clamp(colors + 0.5, min=0.0)

    # the reference's method names, kept so callers/tests written against it keep working
    def project_forward_inputs(self, camera, dims):
        return project_args(self.model, camera, dims, self.device)

    def spherical_harmonics_inputs(self, camera):
        return sh_args(self.model, camera, self.device, self.correct_viewdirs)

    def rasterize_forward_inputs(self, xys, depths, radii, conics, num_tiles, rgbs, dims):
        return raster_args(self.model, xys, depths, radii, conics, num_tiles, rgbs, dims)

    def tile_bounds(self, dims):
        return tile_bounds(dims)
