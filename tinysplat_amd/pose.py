"""Camera pose refinement: a learnable SE(3) correction per training view, the alignment of a
held-out view before it is measured, and relocalisation of a photo against a trained scene.

A view matrix ``V = [R | t]`` (world -> camera, ``R`` orthonormal) is perturbed on the left, ``V(delta) = Exp(delta) V``
with ``delta = (v, omega)`` and ``Exp(delta) = [[exp([omega]x), J(omega) v], [0, 1]]``.  The colour stage gives no gradient
to the view directions, so the loss depends on ``V`` only through the camera-space means and orientations, and its
gradient with respect to ``delta`` at 0 is a fixed linear function of the gradient rows a backward pass leaves on
``means`` and ``quats``: ``dL/dv = sum R g_i``, ``dL/domega = sum (p_i x R g_i + R tau_i)`` (csrc/pose_math.h).  That sum
is one deterministic HIP reduction (``ts_pose_grad``, csrc/pose.hip); nothing here falls back to PyTorch math for it.
What it ignores is the colours' dependence on the pose through the view directions, as the reference's colour stage does.
The six numbers of a view's update, its Adam moments and the retraction live on the host in float64.  The definition
is this project's own: the reference has no pose optimisation and parity with other implementations is not pinned.
"""
from __future__ import annotations

import copy
import ctypes
from dataclasses import asdict, dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _call, _f32c, _need_hip, _ptr, _stream

_SERIES = 0.2                    # below this angle the coefficient that cancels is taken from its series


def _hat(w) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=np.float64)


def _coefficients(theta: float) -> Tuple[float, float, float]:
    """(sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3), each to double rounding at every angle."""
    t2 = theta * theta
    half = 0.5 * theta
    a = np.sin(theta) / theta if theta > 1e-8 else 1.0 - t2 / 6.0
    s = np.sin(half) / half if theta > 1e-8 else 1.0 - t2 / 24.0
    b = 0.5 * s * s                                        # 2 sin^2(t / 2) / t^2: no cancellation
    if theta < _SERIES:
        c = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0 - t2 ** 3 / 362880.0 + t2 ** 4 / 39916800.0
    else:
        c = (theta - np.sin(theta)) / (theta * t2)
    return float(a), float(b), float(c)


def _exp_parts(delta) -> Tuple[np.ndarray, np.ndarray]:
    """(exp([omega]x), J(omega)) of delta = (v, omega)."""
    w = np.asarray(delta, dtype=np.float64).reshape(6)[3:]
    k = _hat(w)
    k2 = k @ k
    a, b, c = _coefficients(float(np.linalg.norm(w)))
    eye = np.eye(3)
    return eye + a * k + b * k2, eye + b * k + c * k2


def se3_exp(delta) -> np.ndarray:
    """delta = (v, omega) in R^6 -> the 4x4 float64 matrix [[exp([omega]x), J(omega) v], [0, 1]] (Rodrigues' formula and
    the left Jacobian in closed form, their coefficients from the series near omega = 0)."""
    delta = np.asarray(delta, dtype=np.float64).reshape(6)
    rot, jac = _exp_parts(delta)
    out = np.eye(4)
    out[:3, :3] = rot
    out[:3, 3] = jac @ delta[:3]
    return out


def _rot_to_quat(rot: np.ndarray) -> np.ndarray:
    """A rotation matrix -> its unit quaternion (w x y z) with w >= 0: the largest of the four squares first."""
    m = np.asarray(rot, dtype=np.float64)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    four = np.array([1.0 + tr, 1.0 + 2.0 * m[0, 0] - tr, 1.0 + 2.0 * m[1, 1] - tr, 1.0 + 2.0 * m[2, 2] - tr])
    i = int(np.argmax(four))
    if i == 0:
        q = np.array([four[0], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    elif i == 1:
        q = np.array([m[2, 1] - m[1, 2], four[1], m[0, 1] + m[1, 0], m[0, 2] + m[2, 0]])
    elif i == 2:
        q = np.array([m[0, 2] - m[2, 0], m[0, 1] + m[1, 0], four[2], m[1, 2] + m[2, 1]])
    else:
        q = np.array([m[1, 0] - m[0, 1], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], four[3]])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _quat_to_rot(q) -> np.ndarray:
    """The rotation matrix of a quaternion (w x y z), normalised first: orthonormal to double rounding."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _quat_mul(a, b) -> np.ndarray:
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dtype=np.float64)


def _quat_log(q) -> np.ndarray:
    """omega of a unit quaternion with w >= 0: 2 atan2(|q_v|, w) q_v / |q_v| (the factor from its series near 0)."""
    q = np.asarray(q, dtype=np.float64)
    s = float(np.linalg.norm(q[1:]))
    if s < 1e-8:
        return 2.0 * q[1:] / q[0]
    return 2.0 * np.arctan2(s, q[0]) / s * q[1:]


def se3_log(T) -> np.ndarray:
    """The inverse of ``se3_exp`` for rotation angles below pi: a 4x4 (or 3x4) rigid transform -> delta = (v, omega)."""
    T = np.asarray(T, dtype=np.float64)
    w = _quat_log(_rot_to_quat(T[:3, :3]))
    _, jac = _exp_parts(np.concatenate([np.zeros(3), w]))
    return np.concatenate([np.linalg.solve(jac, T[:3, 3]), w])


def _exp_quat(w) -> np.ndarray:
    """The unit quaternion of exp([omega]x)."""
    theta = float(np.linalg.norm(w))
    half = 0.5 * theta
    s = np.sin(half) / theta if theta > 1e-8 else 0.5 - theta * theta / 48.0
    return np.array([np.cos(half), s * w[0], s * w[1], s * w[2]], dtype=np.float64)


def retract(quat, trans, delta) -> Tuple[np.ndarray, np.ndarray]:
    """T <- Exp(delta) T for T = [R(quat) | trans]: (the renormalised quaternion, the translation)."""
    delta = np.asarray(delta, dtype=np.float64).reshape(6)
    rot, jac = _exp_parts(delta)
    q = _quat_mul(_exp_quat(delta[3:]), np.asarray(quat, dtype=np.float64))
    return q / np.linalg.norm(q), rot @ np.asarray(trans, dtype=np.float64) + jac @ delta[:3]


def _view34(camera_or_view) -> np.ndarray:
    """The first three rows of a camera's view matrix (or of a matrix given as such) as 12 contiguous float32."""
    vm = getattr(camera_or_view, "view_matrix", camera_or_view)
    if isinstance(vm, Tensor):
        vm = vm.detach().cpu().numpy()
    vm = np.asarray(vm)
    if vm.ndim != 2 or vm.shape[0] < 3 or vm.shape[1] != 4:
        raise ValueError("a view matrix must be [3, 4] or [4, 4]")
    return np.ascontiguousarray(vm[:3, :], dtype=np.float32)


@torch.no_grad()
def pose_gradient(model, camera_or_view, v_means: Optional[Tensor] = None, v_quats: Optional[Tensor] = None) -> Tensor:
    """``ts_pose_grad``: (dL/dv, dL/domega) of the left perturbation of the view matrix the frame was rendered with, a
    float64 [6] tensor on the model's device, from ``model.means``, ``model.quats`` and the gradient rows of a backward
    pass through that frame - ``v_means`` / ``v_quats``, by default ``model.means.grad`` / ``model.quats.grad``.  Raises
    where those are None: a backward pass that applied the fused Adam update wrote no gradient tensors.  The same 48
    bytes on every run."""
    v_means = model.means.grad if v_means is None else v_means
    v_quats = model.quats.grad if v_quats is None else v_quats
    if v_means is None or v_quats is None:
        raise ValueError("pose_gradient needs the gradients of means and quats: run the backward pass without the fused "
                         "Adam update (TrainStep(fused_adam=False), or a step with poses=), which leaves them None")
    means, quats = model.means.detach(), model.quats.detach()
    dev = _need_hip(means, quats, v_means, v_quats)
    n = int(means.shape[0])
    if means.shape != (n, 3) or quats.shape != (n, 4) or v_means.shape != (n, 3) or v_quats.shape != (n, 4):
        raise ValueError("means and v_means must be [N, 3], quats and v_quats [N, 4]")
    means, quats, v_means, v_quats = _f32c(means), _f32c(quats), _f32c(v_means), _f32c(v_quats)
    view = _view34(camera_or_view)
    lib = _lib.load()
    out = torch.empty((6,), dtype=torch.float64, device=dev)
    ws = torch.empty((int(lib.ts_pose_ws_bytes(n)) // 8,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _call("ts_pose_grad", lib.ts_pose_grad, n, view.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(means),
              _ptr(quats), _ptr(v_means), _ptr(v_quats), _ptr(ws) if n else None, _ptr(out), _stream(dev))
    return out


@dataclass
class PoseConfig:
    """Adam on a view's six-vector.  ``lr_translation`` (scene units per step; after ``--normalize-scene`` the scene has
    unit size) and ``lr_rotation`` (radians): the rates of (v, omega); ``weight_decay``: added to the gradient as
    ``weight_decay * Log(T)``, pulling a correction back to the identity.  The three defaults follow gsplat's
    ``pose_opt_lr`` / ``pose_opt_reg`` from memory and are not pinned against it."""
    lr_translation: float = 1e-5
    lr_rotation: float = 1e-5
    weight_decay: float = 1e-6
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-15

    def __post_init__(self):
        self.betas = tuple(float(b) for b in self.betas)
        if self.lr_translation < 0 or self.lr_rotation < 0 or self.weight_decay < 0 or self.eps <= 0:
            raise ValueError("PoseConfig: the rates and the decay must not be negative and eps must be positive")


# what refine_pose and evaluate(refine_poses=K) use when no config is given: a few dozen steps on one frozen scene, not
# tens of thousands of steps beside moving Gaussians
REFINE_CONFIG = dict(lr_translation=2e-3, lr_rotation=2e-3, weight_decay=0.0)

_ORTHONORMAL = 8.0 * 2.0 ** -24      # |R^T R - I| of a float32 rounding of a rotation: three products of two rounded entries


def _base_view(camera) -> np.ndarray:
    """The camera's 4x4 view matrix in float64.  Where its rotation is not orthonormal to float32 rounding it is
    replaced by the nearest rotation (polar factor); a matrix that is orthonormal stays the bits it was."""
    vm = camera.view_matrix
    view = np.eye(4)
    view[:3, :] = np.asarray(vm.detach().cpu().numpy() if isinstance(vm, Tensor) else vm, dtype=np.float64)[:3, :]
    rot = view[:3, :3]
    if np.abs(rot.T @ rot - np.eye(3)).max() > _ORTHONORMAL:
        u, _, vt = np.linalg.svd(rot)
        if np.linalg.det(u @ vt) < 0:
            u[:, 2] = -u[:, 2]
        view[:3, :3] = u @ vt
    return view


class PoseModel:
    """One SE(3) correction ``T_i`` per view, ``V_i = T_i V_i^0``, with Adam's two moments and a step count per view, all
    on the host in float64.  A training step touches the rendered view's entry and nothing else."""

    def __init__(self, cameras: Sequence, config: Optional[PoseConfig] = None):
        self.config = config if config is not None else PoseConfig()
        self.base_cameras = list(cameras)
        if not self.base_cameras:
            raise ValueError("PoseModel: at least one view")
        v = len(self.base_cameras)
        self.base = np.stack([_base_view(c) for c in self.base_cameras])
        self.quats = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (v, 1))
        self.trans = np.zeros((v, 3))
        self.exp_avg = np.zeros((v, 6))
        self.exp_avg_sq = np.zeros((v, 6))
        self.steps = [0] * v
        self._pending = {}               # view -> (pinned host buffer, event): a gradient on its way from the device
        self._free = []                  # pinned 48-byte buffers not in use: as many as were ever in flight together
        self._cameras = [copy.copy(c) for c in self.base_cameras]
        for i in range(v):
            self._refresh(i)

    @property
    def num_views(self) -> int:
        return len(self.base_cameras)

    def _view(self, view) -> int:
        view = int(view)
        if not 0 <= view < self.num_views:
            raise IndexError(f"view {view} of {self.num_views}")
        return view

    def _flush(self, view: Optional[int] = None) -> None:
        """Applies the update whose gradient ``step`` left on its way from the device, for one view or for all."""
        for v in ([view] if view is not None else list(self._pending)):
            waiting = self._pending.pop(v, None)
            if waiting is not None:
                buffer, event = waiting
                event.synchronize()
                self._apply(v, buffer.numpy().copy())
                self._free.append(buffer)

    def _drain(self) -> None:
        """Applies the waiting updates whose copies have arrived, without waiting for any: when an update is applied
        does not change it, and its buffer is free for the next one."""
        for v, (_buffer, event) in list(self._pending.items()):
            if event.query():
                self._flush(v)

    def correction(self, view: int) -> np.ndarray:
        """T_i as a 4x4 float64 matrix."""
        view = self._view(view)
        self._flush(view)
        return self._correction(view)

    def _correction(self, view: int) -> np.ndarray:
        out = np.eye(4)
        out[:3, :3] = _quat_to_rot(self.quats[view])
        out[:3, 3] = self.trans[view]
        return out

    def view_matrix(self, view: int) -> np.ndarray:
        """T_i V_i^0, 4x4 float64."""
        return self.correction(view) @ self.base[self._view(view)]

    def _refresh(self, view: int) -> None:
        # a fresh float32 tensor on the persistent camera object: what rasterizer.camera_on_device memoises on
        self._cameras[view].view_matrix = torch.from_numpy((self._correction(view) @ self.base[view]).astype(np.float32))

    def camera(self, view: int):
        """The view's camera: one persistent shallow copy of the base camera whose ``view_matrix`` is T_i V_i^0 in
        float32, replaced by a new tensor after every update."""
        view = self._view(view)
        self._flush(view)
        return self._cameras[view]

    def cameras(self) -> List:
        """The refined cameras of all views, for export and evaluation."""
        self._flush()
        return list(self._cameras)

    def step(self, view: int, grad6) -> Optional[np.ndarray]:
        """One Adam update of the view's correction from ``grad6`` = ``pose_gradient`` of a frame rendered with
        ``camera(view)``: ``g += weight_decay * Log(T)``, Adam in float64, ``T <- Exp(-lr * m^ / (sqrt(v^) + eps)) T`` with
        the quaternion renormalised.  The gradient is that of the left perturbation at the current pose, so no Jacobian
        of Exp enters.  A host array is applied at once -> the applied six-vector.  A device tensor starts its 48-byte
        copy into pinned host memory and returns None; the update is applied at a later ``step`` once the copy has
        arrived, or when the view is next asked for (``camera(view)``, or anything else that reads the corrections),
        which waits for it - so the host waits only where the same view comes up again at once.  The same numbers
        either way, since nothing reads a correction in between."""
        view = self._view(view)
        self._flush(view)
        self.steps[view] += 1
        if isinstance(grad6, Tensor) and grad6.is_cuda:
            self._drain()
            buffer = self._free.pop() if self._free else torch.empty(6, dtype=torch.float64).pin_memory()
            buffer.copy_(grad6.detach().reshape(6), non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(grad6.device))
            self._pending[view] = (buffer, event)
            return None
        g = grad6.detach().numpy() if isinstance(grad6, Tensor) else np.asarray(grad6)
        return self._apply(view, g)

    def _apply(self, view: int, g) -> np.ndarray:
        cfg = self.config
        g = np.asarray(g).astype(np.float64).reshape(6)
        if cfg.weight_decay != 0.0:
            g = g + cfg.weight_decay * se3_log(self._correction(view))
        t = self.steps[view]
        b1, b2 = cfg.betas
        m = self.exp_avg[view] = b1 * self.exp_avg[view] + (1.0 - b1) * g
        s = self.exp_avg_sq[view] = b2 * self.exp_avg_sq[view] + (1.0 - b2) * g * g
        lr = np.array([cfg.lr_translation] * 3 + [cfg.lr_rotation] * 3)
        delta = -lr * (m / (1.0 - b1 ** t)) / (np.sqrt(s / (1.0 - b2 ** t)) + cfg.eps)
        self.quats[view], self.trans[view] = retract(self.quats[view], self.trans[view], delta)
        self._refresh(view)
        return delta

    def corrections(self) -> np.ndarray:
        """float64 [V, 2]: per view the rotation angle of T_i (radians) and the norm of its translation."""
        self._flush()
        return np.array([[float(np.linalg.norm(_quat_log(q if q[0] >= 0 else -q))), float(np.linalg.norm(t))]
                         for q, t in zip(self.quats, self.trans)]).reshape(-1, 2)

    # ---- persistence
    def state_dict(self) -> dict:
        self._flush()
        return {"config": asdict(self.config), "base": torch.from_numpy(self.base.copy()),
                "quats": torch.from_numpy(self.quats.copy()), "trans": torch.from_numpy(self.trans.copy()),
                "exp_avg": torch.from_numpy(self.exp_avg.copy()), "exp_avg_sq": torch.from_numpy(self.exp_avg_sq.copy()),
                "steps": list(self.steps)}

    def load_state_dict(self, state: dict) -> None:
        if tuple(state["quats"].shape) != tuple(self.quats.shape):
            raise ValueError(f"corrections of {int(state['quats'].shape[0])} views do not fit {self.num_views}")
        saved = state["base"].to(torch.float64).numpy()
        off = np.abs(saved - self.base).reshape(self.num_views, -1).max(axis=1)
        if (off > 1e-6 * np.maximum(1.0, np.abs(self.base).reshape(self.num_views, -1).max(axis=1))).any():
            raise ValueError(f"the corrections were trained on other cameras: view {int(np.argmax(off))}'s base view matrix "
                             f"differs by {off.max():.3g} (another hold-out split, image size or dataset?)")
        self._free.extend(buffer for buffer, _event in self._pending.values())
        self._pending.clear()
        for name in ("quats", "trans", "exp_avg", "exp_avg_sq"):
            setattr(self, name, state[name].to(torch.float64).numpy().copy())
        self.steps = [int(s) for s in state["steps"]]
        for i in range(self.num_views):
            self._refresh(i)

    def save(self, path) -> None:
        torch.save(self.state_dict(), str(path))

    @classmethod
    def load(cls, path, cameras: Sequence) -> "PoseModel":
        """The corrections stored at ``path`` on ``cameras``, the base cameras they were trained on."""
        state = torch.load(str(path), map_location="cpu")
        cfg = dict(state["config"])
        cfg["betas"] = tuple(cfg["betas"])
        model = cls(cameras, PoseConfig(**cfg))
        model.load_state_dict(state)
        return model


class _FixedAffine(torch.autograd.Function):
    """An image through one constant 3x4 colour matrix (a (1, 1, 1) grid of appearance.py); gradient to the image only."""

    @staticmethod
    def forward(ctx, image, grid):
        from .appearance import apply_grid
        image = image.contiguous()
        ctx.save_for_backward(image, grid)
        return apply_grid(image, grid)

    @staticmethod
    def backward(ctx, v_out):
        from .appearance import grid_backward
        image, grid = ctx.saved_tensors
        return grid_backward(image, grid, v_out)[0], None


def refine_pose(model, camera, target: Tensor, device, steps: int = 30, config: Optional[PoseConfig] = None,
                target_depth: Optional[Tensor] = None, appearance_fit: bool = False, background=None,
                lambda_dssim: float = 0.2, lambda_depth: float = 0.2):
    """Aligns ``camera`` to the image ``target`` ([H, W, 3], float32 or uint8) with the Gaussians frozen ->
    ``(camera, history)``: a copy of the camera with the refined ``view_matrix``, and the loss before each of the
    ``steps`` updates.  A step renders under grad, evaluates the training loss (and the depth term where
    ``target_depth`` is given), runs the backward pass without the fused Adam update so that ``means.grad`` and
    ``quats.grad`` exist, reduces them with ``ts_pose_grad``, updates the one pose and drops the gradients unapplied.
    The model is left as found, bit for bit: parameters, requires_grad flags, background, no .grad; a model held by a
    trainer is therefore accepted.  ``config``: by default ``PoseConfig(**REFINE_CONFIG)``; the training defaults are
    sized for thousands of steps.  ``appearance_fit``: each step's render goes through its own least-squares affine
    colour fit to the target (held constant within the step) before the loss, as ``evaluate(color_correct=True)``
    measures.  ``background``: black unless given, as ``evaluate`` renders."""
    from .metrics import affine_color_fit
    from .rasterizer import GaussianRasterizer
    from .training import planes_loss
    dev = torch.device(device)
    poses = PoseModel([camera], config if config is not None else PoseConfig(**REFINE_CONFIG))
    target = target.to(dev)
    if target.dtype == torch.uint8:
        target = target.to(torch.float32) / 255.0
    params = list(model.parameters())
    flags = [p.requires_grad for p in params]
    grads = [p.grad for p in params]
    found = model.background
    render = GaussianRasterizer(model, None, device=dev)
    history: List[float] = []
    try:
        model.background = (torch.zeros(3, device=dev) if background is None
                            else torch.as_tensor(background, dtype=torch.float32).to(dev))
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        with torch.enable_grad():
            for _ in range(int(steps)):
                cam = poses.camera(0)
                rgb, extras = render(cam, None, model.active_sh_degree)
                shown = rgb
                if appearance_fit:
                    fit = torch.from_numpy(affine_color_fit(rgb.detach(), target)).to(torch.float32).reshape(1, 1, 1, 12)
                    shown = _FixedAffine.apply(rgb, fit.to(dev))
                loss = planes_loss(shown.contiguous(), extras["depth"].contiguous(), target, target_depth, lambda_dssim,
                                   lambda_depth)[0]
                loss.backward()
                g = pose_gradient(model, cam)
                for p in params:
                    p.grad = None
                history.append(float(loss.detach()))
                poses.step(0, g)
    finally:
        model.background = found
        for p, flag, grad in zip(params, flags, grads):
            p.grad = grad
            p.requires_grad_(flag)
    return poses.camera(0), history
