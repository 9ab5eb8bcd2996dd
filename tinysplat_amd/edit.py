"""Scene editing: similarity transforms of a model with its spherical harmonics rotated, the matching
move of cameras and point clouds, orientation from the cameras, box crops and merging.

A similarity ``T = (s, R, t)``, ``s > 0`` and ``R`` a proper rotation, maps ``x' = s R x + t``.  Applied to a model:

  means        s R m + t
  scales       scales + log s                              (they are logarithms)
  quats        r (x) q, the Hamilton product with the unit quaternion r of R; the norm of q is kept, no sign rule
  colors_rest  per stored band l and colour channel c'_l = D_l(R) c_l: ALL stored bands, not only the active ones
  colors_dc, opacities   unchanged, the same tensors

``D_l(R)`` is the (2l+1) x (2l+1) matrix with ``sum_j Y_lj(d) D_l[j, k] = Y_lk(R^T d)`` for every unit direction ``d``, in
this project's basis (the 3DGS signs and order of ``ts_sh_fwd``): the colour seen along ``d`` in the new frame is the
colour that was seen along ``R^T d`` in the old one.  The reference has no such function; the definition is this
project's own.

The matching camera keeps its view matrix rigid: ``V' = [R_c R^T | s t_c - R_c R^T t]`` with the projection and the
intrinsics carried over.  Every camera-space point is then ``s`` times what it was: the image is unchanged and the depth
image is multiplied by ``s``.  Two caveats:

  1. near plane: the equality holds up to the near-plane cull, which is an absolute depth;
  2. view directions: the rendered colours are invariant only with ``GaussianRasterizer(..., correct_viewdirs=True)``.  By
     default the adapter reproduces the reference's quirk, SH directions taken from ``view_matrix[:3, 3]``, which is not a
     geometric quantity: no scene transform preserves it.  Degree-0 scenes are invariant either way.

The transform of the Gaussians and the box test run on the GPU (csrc/transform.hip); the rest is host arithmetic in
float64 or plain torch.  No CPU fallback for the two kernels.
"""
from __future__ import annotations

import copy
import ctypes
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _need_hip, _ptr, _stream, deg_from_sh
from .semantic import select_gaussians
from .synthetic import SplatModel

# ------------------------------------------------------------------------------------------------ SH basis, float64
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)
_C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
       -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761)


def sh_band(l: int, dirs: np.ndarray) -> np.ndarray:
    """The 2l+1 basis functions of band l = 1 .. 4 on unit directions [M,3] -> float64 [M, 2l+1] (csrc/sh.h's
    polynomials, the 3DGS signs and order)."""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if l == 1:
        cols = [-_C1 * y, _C1 * z, -_C1 * x]
    elif l == 2:
        cols = [_C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy)]
    elif l == 3:
        cols = [_C3[0] * y * (3.0 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4.0 * zz - xx - yy),
                _C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), _C3[4] * x * (4.0 * zz - xx - yy),
                _C3[5] * z * (xx - yy), _C3[6] * x * (xx - 3.0 * yy)]
    elif l == 4:
        cols = [_C4[0] * xy * (xx - yy), _C4[1] * yz * (3.0 * xx - yy), _C4[2] * xy * (7.0 * zz - 1.0),
                _C4[3] * yz * (7.0 * zz - 3.0), _C4[4] * (zz * (35.0 * zz - 30.0) + 3.0),
                _C4[5] * xz * (7.0 * zz - 3.0), _C4[6] * (xx - yy) * (7.0 * zz - 1.0), _C4[7] * xz * (xx - 3.0 * yy),
                _C4[8] * (xx * (xx - 3.0 * yy) - yy * (3.0 * xx - yy))]
    else:
        raise ValueError("SH bands 1 .. 4")
    return np.stack(cols, axis=-1)


# The directions D_l is solved on: band l uses the first 2l+1 rows, normalised.  Chosen by a seeded search for a small
# condition number of B_l = Y_l(d_j): cond(B_1 .. B_4) = 4.0, 4.8, 3.5, 4.6 (tests/test_transform_cpu.py asserts <= 1e3).
SH_FIT_DIRECTIONS = np.array([
    [-0.86, -0.35, 0.37], [-0.36, -0.54, 0.76], [-0.25, 0.96, -0.16], [-0.42, -0.81, 0.41], [0.41, -0.44, -0.80],
    [0.94, 0.30, 0.17], [-0.06, -0.39, -0.92], [-0.09, -0.90, -0.42], [-0.15, -0.11, 0.98],
], dtype=np.float64)


def _fit_directions(l: int) -> np.ndarray:
    d = SH_FIT_DIRECTIONS[:2 * l + 1]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sh_rotation_matrices(rotation, degree: int) -> List[np.ndarray]:
    """``[D_1, ..., D_degree]``, float64, for a 3x3 rotation: with ``B[j] = Y_l(d_j)`` and ``A[j] = Y_l(R^T d_j)`` on
    2l+1 fixed directions, ``D_l = B^-1 A``.  ``D_l`` is orthogonal and ``D(R2 R1) = D(R2) D(R1)``, both to rounding
    (1e-13); the identity rotation gives identity matrices exactly (the solve would give them to 1e-16), so that an edit
    without rotation leaves every coefficient's bits alone."""
    rot = np.asarray(rotation, dtype=np.float64)
    if rot.shape != (3, 3):
        raise ValueError("rotation must be 3x3")
    if not 0 <= int(degree) <= 4:
        raise ValueError("degree must be 0 .. 4")
    if np.array_equal(rot, np.eye(3)):
        return [np.eye(2 * l + 1) for l in range(1, int(degree) + 1)]
    out = []
    for l in range(1, int(degree) + 1):
        d = _fit_directions(l)
        out.append(np.linalg.solve(sh_band(l, d), sh_band(l, d @ rot)))       # rows of d @ R are (R^T d)^T
    return out


# ------------------------------------------------------------------------------------------------ Sim3
def _quat_to_matrix(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _matrix_to_quat(r: np.ndarray) -> np.ndarray:
    """Unit quaternion (w, x, y, z) of a rotation matrix by the branch with the largest pivot, the sign with w >= 0: the
    quaternions of a rotation and of its inverse are then conjugates, and a transform followed by its inverse gives a
    model's quaternions back with their signs."""
    tr = r[0, 0] + r[1, 1] + r[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s]
    elif r[0, 0] >= r[1, 1] and r[0, 0] >= r[2, 2]:
        s = math.sqrt(1.0 + r[0, 0] - r[1, 1] - r[2, 2]) * 2
        q = [(r[2, 1] - r[1, 2]) / s, 0.25 * s, (r[0, 1] + r[1, 0]) / s, (r[0, 2] + r[2, 0]) / s]
    elif r[1, 1] >= r[2, 2]:
        s = math.sqrt(1.0 + r[1, 1] - r[0, 0] - r[2, 2]) * 2
        q = [(r[0, 2] - r[2, 0]) / s, (r[0, 1] + r[1, 0]) / s, 0.25 * s, (r[1, 2] + r[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + r[2, 2] - r[0, 0] - r[1, 1]) * 2
        q = [(r[1, 0] - r[0, 1]) / s, (r[0, 2] + r[2, 0]) / s, (r[1, 2] + r[2, 1]) / s, 0.25 * s]
    q = np.array(q, dtype=np.float64)
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


@dataclass(frozen=True, eq=False)
class Sim3:
    """The similarity ``x' = scale * rotation @ x + translation``: float64 numpy on the host, frozen.  ``rotation`` is a
    proper rotation (3x3), ``scale`` > 0.  ``a @ b`` applies ``b`` first."""
    rotation: np.ndarray
    translation: np.ndarray
    scale: float

    def __post_init__(self):
        rot = np.array(self.rotation, dtype=np.float64)
        tr = np.array(self.translation, dtype=np.float64).reshape(-1)
        s = float(self.scale)
        if rot.shape != (3, 3) or tr.shape != (3,):
            raise ValueError("rotation must be 3x3 and translation a 3-vector")
        if not (np.isfinite(rot).all() and np.isfinite(tr).all() and math.isfinite(s) and s > 0):
            raise ValueError("a similarity needs finite entries and scale > 0")
        if np.abs(rot.T @ rot - np.eye(3)).max() > 1e-6 or np.linalg.det(rot) <= 0:
            raise ValueError("rotation is not a proper rotation (shear and reflection are not similarities)")
        rot.setflags(write=False)
        tr.setflags(write=False)
        object.__setattr__(self, "rotation", rot)
        object.__setattr__(self, "translation", tr)
        object.__setattr__(self, "scale", s)

    @classmethod
    def identity(cls) -> "Sim3":
        return cls(np.eye(3), np.zeros(3), 1.0)

    @classmethod
    def from_quat(cls, q, translation=(0.0, 0.0, 0.0), scale: float = 1.0) -> "Sim3":
        """``q``: (w, x, y, z), any non-zero norm."""
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        norm = np.linalg.norm(q) if q.shape == (4,) else 0.0
        if not (norm > 0 and math.isfinite(norm)):
            raise ValueError("a quaternion (w, x, y, z) of finite non-zero norm expected")
        return cls(_quat_to_matrix(q / norm), translation, scale)

    @classmethod
    def from_matrix(cls, m4) -> "Sim3":
        """A 4x4 ``[[s R, t], [0 0 0 1]]`` (numpy or torch, float32 or float64).  ValueError unless the last row is
        0 0 0 1 and the upper-left block divided by ``s = det^(1/3)`` is a proper rotation to 1e-6 (max-norm of
        ``R^T R - I``, so the check is relative to the scale): shear, non-uniform scale and reflection are rejected.  The
        rotation kept is the nearest orthogonal matrix."""
        if isinstance(m4, Tensor):
            m4 = m4.detach().cpu().numpy()
        m = np.asarray(m4, dtype=np.float64)
        if m.shape != (4, 4) or not np.isfinite(m).all():
            raise ValueError("a finite 4x4 matrix expected")
        if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("the last row of a similarity is 0 0 0 1")
        det = np.linalg.det(m[:3, :3])
        if not det > 0:
            raise ValueError("the upper-left block has no positive determinant: a reflection or a singular matrix")
        s = det ** (1.0 / 3.0)
        rot = m[:3, :3] / s
        if np.abs(rot.T @ rot - np.eye(3)).max() > 1e-6:
            raise ValueError("the upper-left block is not a scaled rotation (shear or non-uniform scale)")
        u, _, vt = np.linalg.svd(rot)
        return cls(u @ vt, m[:3, 3], s)

    def matrix(self) -> np.ndarray:
        m = np.eye(4)
        m[:3, :3] = self.scale * self.rotation
        m[:3, 3] = self.translation
        return m

    def quat(self) -> np.ndarray:
        """The unit quaternion (w, x, y, z) of the rotation."""
        return _matrix_to_quat(self.rotation)

    def inverse(self) -> "Sim3":
        rt = self.rotation.T
        return Sim3(rt, -(rt @ self.translation) / self.scale, 1.0 / self.scale)

    def __matmul__(self, other: "Sim3") -> "Sim3":
        if not isinstance(other, Sim3):
            return NotImplemented
        return Sim3(self.rotation @ other.rotation,
                    self.scale * (self.rotation @ other.translation) + self.translation, self.scale * other.scale)

    def apply(self, points) -> np.ndarray:
        """float64 [..., 3] -> ``s R x + t``."""
        p = np.asarray(points, dtype=np.float64)
        return self.scale * (p @ self.rotation.T) + self.translation


# ------------------------------------------------------------------------------------------------ the Gaussians
def kernel_arguments(sim3: Sim3, degree: int):
    """The float32 host arrays ``ts_transform_gaussians`` receives -> ``(xform [12], quat [4], log_scale, sh [..])``:
    M = fl32(s R) row-major then fl32(t), the unit quaternion, fl32(log s), D_1 | .. | D_degree row-major."""
    xform = np.concatenate([(sim3.scale * sim3.rotation).reshape(-1), sim3.translation]).astype(np.float32)
    quat = sim3.quat().astype(np.float32)
    log_scale = float(np.float32(math.log(sim3.scale)))
    mats = sh_rotation_matrices(sim3.rotation, degree)
    sh = np.concatenate([m.reshape(-1) for m in mats]).astype(np.float32) if mats else np.zeros(0, np.float32)
    return xform, quat, log_scale, sh


def _float_array(a: np.ndarray):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _refuse_held(model, what: str) -> None:
    if getattr(model, "held_by", None):
        raise RuntimeError(f"{what} on a model held by {sorted(model.held_by)}: the optimiser state of its rows is not "
                           "transformed with them; edit the scene before training or after it")


@torch.no_grad()
def transform_gaussians(model, sim3: Sim3, mask: Optional[Tensor] = None) -> SplatModel:
    """The model moved by ``sim3`` (module docstring) as a new ``SplatModel``: new tensors for means, scales, quats and
    colors_rest, the same tensors for colors_dc and opacities, the same ``active_sh_degree`` and ``background``.  The
    input is not written.  ``mask``: bool [N] on the model's device; rows where it is false come out with the input's
    bits, so one object (a class of ``lift_labels``, say) can be moved.  One launch (csrc/transform.hip).  Refuses a
    model held by a trainer and CPU tensors.  The render is invariant under the matching ``transform_camera`` only up to
    the near-plane cull and only with ``correct_viewdirs=True`` (module docstring)."""
    if not isinstance(sim3, Sim3):
        raise TypeError("sim3 must be a Sim3")
    _refuse_held(model, "transform_gaussians")
    means, scales, quats, rest = (_f32c(getattr(model, f).detach()) for f in ("means", "scales", "quats", "colors_rest"))
    dev = _need_hip(means, scales, quats, rest)
    n, k_rest = int(means.shape[0]), int(rest.shape[1])
    degree = deg_from_sh(k_rest + 1)
    if mask is not None:
        if not isinstance(mask, Tensor) or mask.dtype != torch.bool or mask.shape != (n,):
            raise ValueError("mask must be a bool [N] tensor")
        _need_hip(means, mask)
        mask = mask.contiguous()
    xform, quat, log_scale, sh = kernel_arguments(sim3, degree)
    (xform, xform_p), (quat, quat_p), (sh, sh_p) = _float_array(xform), _float_array(quat), _float_array(sh)
    out = [torch.empty_like(t) for t in (means, scales, quats, rest)]
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_transform_gaussians", lib.ts_transform_gaussians, n, k_rest, xform_p, quat_p, log_scale,
              sh_p if sh.size else None, _ptr(mask) if mask is not None and n else None,
              *[_ptr(t) if t.numel() else None for t in (means, scales, quats, rest)],
              *[_ptr(t) if t.numel() else None for t in out], _stream(dev))
    return SplatModel(out[0], model.colors_dc, out[3], out[1], out[2], model.opacities,
                      active_sh_degree=model.active_sh_degree, background=model.background,
                      rasterize_mode=getattr(model, "rasterize_mode", "classic"))


def transform_points(points: Tensor, sim3: Sim3) -> Tensor:
    """``s R x + t`` on a [M,3] tensor in its own dtype and on its own device (an SfM cloud before ``from_pcd``).  Plain
    torch."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points [M,3] expected")
    m = torch.as_tensor(sim3.scale * sim3.rotation, dtype=points.dtype, device=points.device)
    t = torch.as_tensor(np.array(sim3.translation), dtype=points.dtype, device=points.device)
    return points @ m.T + t


# ------------------------------------------------------------------------------------------------ cameras
def transform_camera(camera, sim3: Sim3):
    """A new camera that sees the transformed scene as ``camera`` saw the original one: ``V' = [R_c R^T | s t_c - R_c R^T
    t]``, built in float64 and stored float32; the projection matrix, ``f_x``, ``f_y``, ``width``, ``height`` and the
    field-of-view angles are carried over.  Camera-space points are ``s`` times what they were: the same image, depth
    times ``s`` (up to the near-plane cull; colours only with ``correct_viewdirs=True``, module docstring)."""
    v = camera.view_matrix.detach().cpu().numpy().astype(np.float64)
    rot = v[:3, :3] @ sim3.rotation.T
    out = np.eye(4)
    out[:3, :3] = rot
    out[:3, 3] = sim3.scale * v[:3, 3] - rot @ sim3.translation
    new = copy.copy(camera)
    new.view_matrix = torch.as_tensor(out, dtype=torch.float32)
    if getattr(camera, "position", None) is not None:            # a dataset camera keeps its centre (dataset.py)
        new.position = sim3.apply(np.asarray(camera.position, dtype=np.float64))
    return new


def transform_cameras(cameras: Sequence, sim3: Sim3) -> list:
    return [transform_camera(c, sim3) for c in cameras]


def orient_from_cameras(cameras: Sequence, up=(0.0, 0.0, 1.0), center: bool = True, unit_scale: bool = True) -> Sim3:
    """The similarity that turns the cameras' mean up direction to ``up``, puts the mean camera centre at the origin
    (``center``) and the farthest camera at distance 1 from it (``unit_scale``); float64 on the host.  Centres are
    ``c_i = -R_i^T t_i``, world up is ``normalise(sum_i -R_i^T e_y)`` (the image y axis points down).  The rotation is
    the minimal one taking that to ``up``: the identity if the sum is shorter than 1e-8 per camera, and for the
    opposite direction a half turn about ``normalise(up x e_a)``, ``e_a`` the coordinate axis with the smallest
    ``|up_a|`` (lowest index on ties).  The scale is 1 for a single camera."""
    if len(cameras) == 0:
        raise ValueError("orient_from_cameras needs at least one camera")
    up = np.asarray(up, dtype=np.float64).reshape(-1)
    if up.shape != (3,) or not np.linalg.norm(up) > 0:
        raise ValueError("up must be a non-zero 3-vector")
    up = up / np.linalg.norm(up)
    views = [c.view_matrix.detach().cpu().numpy().astype(np.float64) for c in cameras]
    centres = np.stack([-(v[:3, :3].T @ v[:3, 3]) for v in views])
    total = np.sum([-v[:3, :3].T[:, 1] for v in views], axis=0)
    norm = np.linalg.norm(total)
    rot = np.eye(3)
    if norm >= 1e-8 * len(views):
        u = total / norm
        axis, cos = np.cross(u, up), float(u @ up)
        sin = np.linalg.norm(axis)
        if sin < 1e-12 and cos < 0:                                   # opposite: a half turn about an axis normal to up
            a = int(np.argmin(np.abs(up)))
            k = np.cross(up, np.eye(3)[a])
            k = k / np.linalg.norm(k)
            rot = 2.0 * np.outer(k, k) - np.eye(3)
        elif sin >= 1e-12:
            k = axis / sin
            kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            rot = np.eye(3) + sin * kx + (1.0 - cos) * (kx @ kx)
    mean = centres.mean(axis=0) if center else np.zeros(3)
    spread = np.linalg.norm(centres - centres.mean(axis=0), axis=1).max()
    scale = 1.0 / spread if unit_scale and len(views) > 1 and spread > 0 else 1.0
    return Sim3(rot, -scale * (rot @ mean), scale)


# ------------------------------------------------------------------------------------------------ crop, merge
@torch.no_grad()
def box_mask(model, center, half_extent, rotation=None) -> Tensor:
    """bool [N] on the model's device: ``|R_box^T (m - center)|_i <= half_extent_i`` on all three axes, evaluated in
    float32 as ``|A m + b|_i <= 1`` with ``A = diag(1 / half_extent) R_box^T`` and ``b = -A center`` rounded from float64
    (csrc/transform.hip).  ``rotation``: the box's axes as columns (3x3), default the world's.  NaN means are outside."""
    c = np.asarray(center, dtype=np.float64).reshape(-1)
    h = np.asarray(half_extent, dtype=np.float64).reshape(-1)
    rot = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64)
    if c.shape != (3,) or h.shape != (3,) or rot.shape != (3, 3):
        raise ValueError("center and half_extent are 3-vectors, rotation is 3x3")
    if not (np.isfinite(c).all() and np.isfinite(h).all() and (h > 0).all() and np.isfinite(rot).all()):
        raise ValueError("a box needs a finite centre and rotation and half extents > 0")
    a = rot.T / h[:, None]
    box, box_p = _float_array(np.concatenate([a.reshape(-1), -(a @ c)]))
    means = _f32c(model.means.detach())
    dev = _need_hip(means)
    n = int(means.shape[0])
    inside = torch.empty((n,), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _call("ts_box_mask", lib.ts_box_mask, n, box_p, _ptr(means) if n else None, _ptr(inside) if n else None,
              _stream(dev))
    return inside.view(torch.bool)


def crop_gaussians(model, center, half_extent, rotation=None) -> SplatModel:
    """``select_gaussians`` on ``box_mask``: the Gaussians whose mean is inside the box, rows in order."""
    return select_gaussians(model, box_mask(model, center, half_extent, rotation))


def merge_models(models: Sequence) -> SplatModel:
    """The models' rows concatenated in order.  ``colors_rest`` is zero-padded to the largest stored degree,
    ``active_sh_degree`` is the maximum, ``background`` the first model's.  Plain torch; raises on an empty list or
    models on different devices, or of different rasterize modes (an opacity means something else in each)."""
    models = list(models)
    if not models:
        raise ValueError("merge_models needs at least one model")
    modes = {getattr(m, "rasterize_mode", "classic") for m in models}
    if len(modes) > 1:
        raise ValueError(f"merge_models: the models have different rasterize modes {sorted(modes)}")
    dev = models[0].means.device
    if any(p.device != dev for m in models for p in m.parameters()):
        raise ValueError("merge_models: the models live on different devices")
    k_rest = max(int(m.colors_rest.shape[1]) for m in models)
    deg_from_sh(k_rest + 1)
    rests = []
    for m in models:
        r = m.colors_rest.detach()
        pad = r.new_zeros((r.shape[0], k_rest - r.shape[1], 3))
        rests.append(torch.cat([r, pad], dim=1))
    cat = {f: torch.cat([getattr(m, f).detach() for m in models], dim=0)
           for f in ("means", "colors_dc", "scales", "quats", "opacities")}
    return SplatModel(cat["means"], cat["colors_dc"], torch.cat(rests, dim=0), cat["scales"], cat["quats"],
                      cat["opacities"], active_sh_degree=max(int(m.active_sh_degree) for m in models),
                      background=models[0].background, rasterize_mode=modes.pop())
