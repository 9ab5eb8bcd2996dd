"""Inputs shared by tests/test_pose_cpu.py and tests/test_gpu_pose.py: gradient rows for the reduction, the g++ build of
tests/hostmath/pose.cpp, the small scene whose pose gradient the float64 oracle differentiates, and the offset cameras
of the refinement tests."""
import ctypes
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

import pose_oracle as PO

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
F32P = ctypes.POINTER(ctypes.c_float)
F64P = ctypes.POINTER(ctypes.c_double)

# n of the reduction checks: nothing, one row, around a wave's 64 lanes, one row into a workgroup's second wave (a wave
# owns 256 rows, a workgroup 1024), one row past four workgroups; MANY leaves 1025 records, one more than the second pass
# has slots
SIZES = (0, 1, 63, 64, 65, 257, 4097)
MANY = 1024 * 1024 + 1


def quat_to_rot(q):
    """Rotation matrix of a quaternion (w x y z) that is normalised first, float64."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def view_matrix(quat=(0.97, 0.06, -0.12, 0.09), position=(0.3, -0.2, -0.5)):
    """4x4 float64 world -> camera matrix [R | -R p] of a normalised quaternion."""
    view = np.eye(4)
    view[:3, :3] = quat_to_rot(quat)
    view[:3, 3] = -view[:3, :3] @ np.asarray(position, dtype=np.float64)
    return view


def random_rows(n, seed, zero="none"):
    """float32 (means N(0, 3), quats N(0, 1.7), v_means N(0, 1) x 10^U(-3, 1), v_quats likewise) of n rows.  ``zero``:
    "ends": the gradient rows at both ends and across row 64 are zero (culled Gaussians); "all": every gradient row."""
    g = np.random.default_rng(seed)
    means = (3.0 * g.normal(size=(n, 3))).astype(np.float32)
    quats = (1.7 * g.normal(size=(n, 4))).astype(np.float32)
    v_means = (g.normal(size=(n, 3)) * 10.0 ** g.uniform(-3, 1, size=(n, 1))).astype(np.float32)
    v_quats = (g.normal(size=(n, 4)) * 10.0 ** g.uniform(-3, 1, size=(n, 1))).astype(np.float32)
    if zero == "all":
        v_means[:], v_quats[:] = 0.0, 0.0
    elif zero == "ends":
        for lo, hi in ((0, 7), (60, 70), (n - 9, n)):
            lo, hi = max(0, lo), min(n, hi)
            v_means[lo:hi], v_quats[lo:hi] = 0.0, 0.0
    return means, quats, v_means, v_quats


def build_host(directory):
    """g++ build of tests/hostmath/pose.cpp: the kernel's header compiled for the host."""
    so = Path(directory) / "_pose.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "pose.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.ph_pose_grad.restype, lib.ph_pose_grad.argtypes = None, [ctypes.c_int64, F32P, F32P, F32P, F32P, F32P, F64P]
    lib.ph_pose_row.restype, lib.ph_pose_row.argtypes = None, [F32P, F32P, F32P, F32P, F32P, F64P]
    return lib


def _f(a):
    return a.ctypes.data_as(F32P)


def host_pose_grad(lib, view, means, quats, v_means, v_quats):
    """The host build on n rows -> float64 [6]."""
    arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in (means, quats, v_means, v_quats)]
    view = np.ascontiguousarray(np.asarray(view)[:3, :], dtype=np.float32)
    out = np.full(6, 7.0)
    lib.ph_pose_grad(arrays[0].shape[0], _f(view), *[_f(a) for a in arrays], out.ctypes.data_as(F64P))
    return out


def rounding_bound(view, means, quats, v_means, v_quats):
    """How far two float64 evaluations of the six sums may differ, u = 2^-53.  A component of one row is a sum of
    products of float32 values nested at most ten operations deep (p: a product and three sums; p x gc: a product and
    a difference more on two such chains; R tau: four operations for tau, three for the product and sums; the final
    sum), so each of the two evaluations is within 10 u (1 + O(u)) of the exact row term, measured against the sum of
    the absolute products ``magnitude``.  Adding n such terms in any order moves the result by at most (n - 1) u times
    the sum of their absolute values, and the oracle's exactly rounded sum by u.  Together, with a factor 2 for the
    second-order terms: (n + 24) 2^-52 magnitude per component."""
    n = np.asarray(means).shape[0]
    return (n + 24) * 2.0 ** -52 * PO.magnitude(np.asarray(view, dtype=np.float32), means, quats, v_means, v_quats)


# ---- the scene of the identity check: 60 Gaussians, 48 x 32 pixels, degree 0
WIDTH, HEIGHT, N_SCENE = 48, 32, 60
FOV_X = math.radians(60.0)


def intrinsics(width=WIDTH, height=HEIGHT):
    fx = width / (2.0 * math.tan(FOV_X / 2.0))
    fov_y = 2.0 * math.atan(height / (2.0 * fx))
    proj = np.zeros((4, 4))
    znear, zfar = 0.001, 1000.0
    proj[0, 0], proj[1, 1] = 1.0 / math.tan(FOV_X / 2), 1.0 / math.tan(fov_y / 2)
    proj[2, 2], proj[2, 3], proj[3, 2] = (zfar + znear) / (zfar - znear), -zfar * znear / (zfar - znear), 1.0
    return fx, fx, proj


def small_scene(seed=5):
    """float32 arrays of a 60-Gaussian model placed in front of ``view_matrix()``: raw quaternions of norm about 1.7
    |randn|, rows 0..2 beyond the 1.3 fov clamp but wide enough to reach the image, row 3 behind the camera."""
    g = np.random.default_rng(seed)
    n = N_SCENE
    tan_x, tan_y = math.tan(FOV_X / 2), HEIGHT / WIDTH * math.tan(FOV_X / 2)
    z = g.uniform(2.0, 8.0, size=n)
    x = z * tan_x * g.uniform(-1.2, 1.2, size=n)
    y = z * tan_y * g.uniform(-1.2, 1.2, size=n)
    sigma = z[:, None] * g.uniform(0.02, 0.08, size=(n, 3))
    x[:3] = z[:3] * tan_x * np.array([1.42, -1.38, 1.45])
    y[:3] = z[:3] * tan_y * np.array([0.2, -0.4, 1.36])
    sigma[:3] = z[:3, None] * g.uniform(0.12, 0.2, size=(3, 3))
    z[3] = -1.0
    view = view_matrix()
    cam_pts = np.stack([x, y, z], axis=1)
    means = (cam_pts - view[:3, 3]) @ view[:3, :3]                 # R^T (p - t)
    return {"means": means.astype(np.float32), "scales": np.log(sigma).astype(np.float32),
            "quats": (1.7 * g.normal(size=(n, 4))).astype(np.float32),
            "opacities": (1.5 * g.normal(size=(n, 1))).astype(np.float32),
            "colors_dc": g.normal(size=(n, 3)).astype(np.float32)}


def oracle_pose_run(scene, view, width=WIDTH, height=HEIGHT, w_rgb=None, w_d=None, target=None):
    """The weighted RGB + depth loss of ``scene`` (with ``target``, a float64 [H, W, 3] tensor: the training loss
    0.8 L1 + 0.2 (1 - SSIM) of oracle/train_oracle.py against it) through oracle/gsplat_oracle.py in float64 with the 4x4 view matrix as
    the differentiated leaf (viewmat and projmat = P @ V both built from it) -> dict: ``pose`` = autograd's gradient of
    the left perturbation Exp(delta) V at 0 (dL/dv = G[:, 3], dL/domega = sum_j V[:, j] x G[:, j] over the four columns of
    G = dL/dV[:3]), ``v_means`` / ``v_quats`` = the oracle's own gradient rows, ``clamped`` / ``culled``: rows beyond the
    fov clamp that hit a tile / rows with no tile."""
    from oracle import gsplat_oracle as O
    from tinysplat_amd.synthetic import loss_weights
    fx, fy, proj = intrinsics(width, height)
    if w_rgb is None and target is None:
        w_rgb, w_d = loss_weights(width, height)
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in scene.items()}
    V = torch.tensor(np.asarray(view, dtype=np.float64), requires_grad=True)
    P = torch.tensor(proj)
    tb = (-(-width // 16), -(-height // 16), 1)
    unit = t["quats"] / t["quats"].norm(dim=-1, keepdim=True)
    xys, depths, radii, conics, nth, _ = O.project_gaussians(t["means"], torch.exp(t["scales"]), 1.0, unit, V[:3, :], P @ V,
                                                             fx, fy, width / 2, height / 2, height, width, tb)
    dirs = t["means"].detach() - V[:3, 3].detach()
    col = torch.clamp(O.spherical_harmonics(0, dirs / dirs.norm(dim=-1, keepdim=True), t["colors_dc"][:, None, :]) + 0.5,
                      min=0.0)
    bg = torch.zeros(3, dtype=torch.float64)
    op = torch.sigmoid(t["opacities"])
    img, _ = O.rasterize_gaussians(xys, depths, radii, conics, nth, col, op, height, width, bg)
    dimg, _ = O.rasterize_gaussians(xys, depths, radii, conics, nth, depths[:, None].repeat(1, 3), op, height, width, bg)
    if target is not None:
        from oracle.train_oracle import photometric_loss
        loss = photometric_loss(torch.clamp(img, max=1.0), target)
        loss = loss[0] if isinstance(loss, tuple) else loss
    else:
        loss = (torch.clamp(img, max=1.0) * w_rgb.double()).sum() + (dimg[:, :, 0] * w_d.double()).sum()
    loss.backward()
    G, Vn = V.grad.numpy()[:3, :], V.detach().numpy()[:3, :]
    pose = np.concatenate([G[:, 3], sum(np.cross(Vn[:, j], G[:, j]) for j in range(4))])
    cam = t["means"].detach().numpy() @ Vn[:, :3].T + Vn[:, 3]
    limx, limy = 1.3 * (0.5 * width) / fx, 1.3 * (0.5 * height) / fy
    beyond = (cam[:, 2] > 0.01) & ((np.abs(cam[:, 0] / cam[:, 2]) > limx) | (np.abs(cam[:, 1] / cam[:, 2]) > limy))
    hit = nth.numpy() > 0
    return {"pose": pose, "loss": float(loss.detach()),"v_means": t["means"].grad.numpy(), "v_quats": t["quats"].grad.numpy(),
            "clamped": beyond & hit, "culled": ~hit, "image": torch.clamp(img, max=1.0).detach()}


@functools.lru_cache(maxsize=None)
def small_scene_reference():
    """(scene, view, oracle_pose_run(scene, view)) of the identity check, computed once per process."""
    scene, view = small_scene(), view_matrix()
    return scene, view, oracle_pose_run(scene, view)


def camera_from_view(view, width, height):
    """A PinholeCamera of the check's intrinsics with the float32 rounding of ``view``."""
    from tinysplat_amd.synthetic import PinholeCamera
    fx, fy, proj = intrinsics(width, height)
    return PinholeCamera(torch.as_tensor(np.asarray(view), dtype=torch.float32), torch.as_tensor(proj, dtype=torch.float32),
                         fx, fy, width, height)


def model_from_scene(scene, device):
    from tinysplat_amd.synthetic import SplatModel
    n = scene["means"].shape[0]
    t = {k: torch.from_numpy(v.copy()) for k, v in scene.items()}
    return SplatModel(t["means"], t["colors_dc"], torch.zeros((n, 0, 3)), t["scales"], t["quats"], t["opacities"], 0,
                      background=torch.zeros(3)).to(device)


# ---- the offset of the refinement tests: 0.01 rad about a skew axis, 1 % of the camera-to-scene distance
OFFSET_AXIS = np.array([0.48, -0.6, 0.64])              # unit
OFFSET_ANGLE = 0.01
OFFSET_DIRECTION = np.array([0.6, 0.64, -0.48])         # unit


def offset_view(view_true, distance, sign=1.0):
    """The 4x4 float64 view matrix Exp(delta) V_true with delta = sign (0.01 distance e, 0.01 a)."""
    from tinysplat_amd.pose import se3_exp
    delta = sign * np.concatenate([0.01 * distance * OFFSET_DIRECTION, OFFSET_ANGLE * OFFSET_AXIS])
    return se3_exp(delta) @ np.asarray(view_true, dtype=np.float64)


# the refinement case: make_scene(REFINE_N, 0, 160, 120, scale_mult = REFINE_SCALE) seen from the origin; the rates and the
# step count are chosen for this case (PoseConfig's defaults are sized for training)
REFINE_N, REFINE_DIMS, REFINE_SCALE, REFINE_SEED = 3000, (160, 120), 8.0, 3
REFINE_STEPS, REFINE_LR_T, REFINE_LR_R = 60, 2e-3, 4e-4


def refine_scene(n=REFINE_N, dims=REFINE_DIMS):
    """(model, camera, mean depth) of the refinement case, or of a reduced copy of it (fewer Gaussians on fewer pixels
    at the same field of view: the same picture at a lower resolution)."""
    from tinysplat_amd.synthetic import make_scene
    model, cam = make_scene(n, 0, dims[0], dims[1], seed=REFINE_SEED, scale_mult=REFINE_SCALE)
    return model, cam, float(model.means[:, 2].mean())


def oracle_refine(model, cam, distance, steps=REFINE_STEPS, lr_t=REFINE_LR_T, lr_r=REFINE_LR_R, report=None):
    """refine_pose's loop in float64 on the CPU: oracle render and loss, pose_oracle's six sums and Adam retraction.
    -> (angle ratio, translation ratio) of the final to the initial pose error."""
    w, h = cam.width, cam.height
    scene = {"means": model.means.numpy(), "scales": model.scales.numpy(), "quats": model.quats.numpy(),
             "opacities": model.opacities.numpy(), "colors_dc": model.colors_dc.numpy()}
    true = cam.view_matrix.double().numpy()
    start = offset_view(true, distance)
    target = oracle_pose_run(scene, true, w, h)["image"]
    T, m, v = np.eye(4), np.zeros(6), np.zeros(6)
    first = PO.pose_error(true, start)
    for step in range(1, steps + 1):
        run = oracle_pose_run(scene, T @ start, w, h, target=target)
        g = PO.pose_gradient(T @ start, scene["means"], scene["quats"], run["v_means"], run["v_quats"])
        T, m, v = PO.adam_retraction(T, m, v, step, g, [lr_t] * 3 + [lr_r] * 3)
        if report is not None:
            report(step, run["loss"], PO.pose_error(true, T @ start))
    last = PO.pose_error(true, T @ start)
    return last[0] / first[0], last[1] / first[1]
