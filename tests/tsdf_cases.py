"""The inputs of the fusion's tests (tests/test_tsdf_cpu.py, tests/test_gpu_tsdf.py): the smallest
at which each part can still go wrong.  Grids of 24^3 cells (27 bricks) and 20 x 17 x 9 cells (partial bricks on every
axis); images of 48 x 40 and one camera of 32 x 32 in the same list; 1, 2 and 7 cameras, one of them inside the volume
with part of the grid behind it; analytic depth maps of a tilted plane (with a band of rows without depth and a NaN pixel)
and of a sphere seen by six axis cameras; trunc of 2 h and 4 h; min_observations of 1 and 2.  The oracle runs once per case
and is shared."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import tsdf_oracle as TO

PLANE_N = np.array([0.3, 0.2, 1.0]) / math.sqrt(0.3 ** 2 + 0.2 ** 2 + 1.0)
PLANE_C = 0.137
SPHERE_C = np.array([0.031, -0.023, 0.047])
SPHERE_R = 1.0
CUBE = ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2))                # 24^3 cells of h = 0.1
SLAB = ((-1.0, -0.85, -0.33), (1.0, 0.849, 0.569))           # 20 x 17 x 9 cells of h = 0.1


def look_at(position, target, width, height, fov_x_deg=60.0, up=(0.0, 1.0, 0.0), znear=0.001, zfar=1000.0):
    """A pinhole camera at ``position`` looking along +z of its own frame at ``target`` -> (view, proj) float32 [4,4], the
    matrices of tinysplat_amd.synthetic.PinholeCamera."""
    p, t = np.asarray(position, np.float64), np.asarray(target, np.float64)
    f = (t - p) / np.linalg.norm(t - p)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    rot = np.stack((r, u, f))
    view = np.eye(4)
    view[:3, :3] = rot
    view[:3, 3] = -rot @ p
    fov_x = math.radians(fov_x_deg)
    f_x = width / (2.0 * math.tan(fov_x / 2.0))
    fov_y = 2.0 * math.atan(height / (2.0 * f_x))
    proj = np.zeros((4, 4))
    proj[0, 0] = 1.0 / math.tan(fov_x / 2)
    proj[1, 1] = 1.0 / math.tan(fov_y / 2)
    proj[2, 2] = (zfar + znear) / (zfar - znear)
    proj[2, 3] = -zfar * znear / (zfar - znear)
    proj[3, 2] = 1
    return view.astype(np.float32), proj.astype(np.float32)


def pixel_rays(view, proj, width, height):
    """(origin [3], directions [H,W,3] with view-space z = 1) of the pixel centres, float64, from the float32 matrices."""
    v, p = view.astype(np.float64), proj.astype(np.float64)
    nx = (np.arange(width) + 0.5 - 0.5 * width) * 2.0 / width
    ny = (np.arange(height) + 0.5 - 0.5 * height) * 2.0 / height
    dv = np.stack(np.broadcast_arrays(nx[None, :] / p[0, 0], ny[:, None] / p[1, 1], np.ones((height, width))), -1)
    rot = v[:3, :3]
    return -rot.T @ v[:3, 3], dv @ rot                       # R^T dir = dir @ R


def plane_depth(view, proj, width, height):
    o, d = pixel_rays(view, proj, width, height)
    with np.errstate(divide="ignore"):
        z = (PLANE_C - PLANE_N @ o) / (d @ PLANE_N)
    return np.where(np.isfinite(z) & (z > 0), z, 0.0).astype(np.float32)


def sphere_depth(view, proj, width, height):
    o, d = pixel_rays(view, proj, width, height)
    oc = o - SPHERE_C
    a, b, c = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        z = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (z > 0), z, 0.0).astype(np.float32)


def _camera(position, target, width, height, depth_fn, **kw):
    view, proj = look_at(position, target, width, height, **kw)
    return {"view": view, "proj": proj, "depth": depth_fn(view, proj, width, height), "width": width, "height": height}


@functools.lru_cache(maxsize=None)
def plane_cameras():
    """Seven cameras above the plane: 48 x 40 but the third (32 x 32); the fifth sits inside the volume, so part of the grid
    is behind it; the first map has a band of rows without depth and a NaN pixel."""
    spots = [((0.21, -0.13, 2.9), (0.0, 0.0, 0.1)), ((1.7, 0.4, 2.3), (0.1, 0.0, 0.1)), ((-1.1, 1.3, 2.5), (0.0, 0.1, 0.1)),
             ((0.3, -1.9, 2.2), (0.0, -0.1, 0.1)), ((0.25, 0.15, 0.95), (0.05, -0.05, 0.1)), ((-1.6, -1.0, 2.0), (0.0, 0.0, 0.2)),
             ((0.9, 1.5, 2.6), (0.1, 0.1, 0.0))]
    cams = []
    for i, (p, t) in enumerate(spots):
        w, h = (32, 32) if i == 2 else (48, 40)
        # rolled about its axis: a camera whose image axes follow the grid's puts whole rows of corners on a pixel border
        up = (0.31 - 0.17 * i, 1.0, 0.23 * (i % 3) - 0.19)
        cams.append(_camera(p, t, w, h, plane_depth, fov_x_deg=50.0 if i != 4 else 80.0, up=up))
    cams[0]["depth"][17:20, :] = 0.0
    cams[0]["depth"][9, 31] = np.nan
    cams[0]["depth"][30, 5] = -1.0
    return tuple(cams)


@functools.lru_cache(maxsize=None)
def sphere_cameras():
    out = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            p = np.zeros(3)
            p[axis] = 30.0 * sign
            up = (0.13, 1.0, 0.29) if axis != 1 else (0.21, 0.17, 1.0)
            # 30 away: far enough that a ray meets the surface at most 60 degrees off the normal anywhere between two axes: a corner
            # of a crossed cell, up to sqrt(3) h inside, then lies less than trunc = 4 h behind the surface along the ray;
            # and the sphere large enough that a corner sqrt(3) h outside it between three axes (sqrt(2 / 3) of its
            # radius off each) still projects into a silhouette: 1.2247 R - R > sqrt(3) h
            out.append(_camera(p + (0.011, 0.007, -0.013), (0.0, 0.0, 0.0), 48, 40, sphere_depth, fov_x_deg=4.95, up=up))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def narrow_cameras():
    """Two cameras of a narrow view on two spots of the plane, the first inside the volume: most bricks are outside either
    frustum, which is what the integration's sphere test skips."""
    return (_camera((-0.71, -0.62, 1.1), (-0.66, -0.6, 0.0), 48, 40, plane_depth, fov_x_deg=24.0, up=(0.31, 1.0, -0.19)),
            _camera((0.63, 0.52, 2.1), (0.6, 0.5, 0.1), 32, 32, plane_depth, fov_x_deg=16.0, up=(-0.2, 1.0, 0.27)))


@functools.lru_cache(maxsize=None)
def front_camera():
    """One camera looking along -PLANE_N at the plane from 2.5 away: the depth is the same in every pixel, the field is
    linear in the corner, and the interpolated vertices lie on the plane."""
    cam = _camera(tuple(PLANE_C * PLANE_N + 2.5 * PLANE_N), tuple(PLANE_C * PLANE_N), 48, 40, plane_depth, fov_x_deg=50.0,
                  up=(0.31, 1.0, -0.19))
    cam["depth"] = np.full((40, 48), 2.5, dtype=np.float32)
    return (cam,)


# name -> (bounds, resolution, cameras, trunc_voxels, min_observations)
CASES = {
    "front": (CUBE, 24, lambda: front_camera(), 4.0, 1),
    "plane1": (CUBE, 24, lambda: plane_cameras()[:1], 4.0, 1),
    "plane2": (CUBE, 24, lambda: plane_cameras()[:2], 4.0, 1),
    "plane7": (CUBE, 24, lambda: plane_cameras(), 4.0, 1),
    "plane7_thin": (CUBE, 24, lambda: plane_cameras(), 2.0, 2),
    "narrow2": (CUBE, 24, lambda: narrow_cameras(), 4.0, 1),
    "slab3": (SLAB, 20, lambda: plane_cameras()[:3], 2.0, 2),
    "sphere": (CUBE, 24, lambda: sphere_cameras(), 4.0, 1),
}
ZNEAR = 0.001


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs and the oracle's run of a case, computed once and left unchanged."""
    import mesh_oracle as MO
    bounds, res, cams, tv, min_obs = CASES[name]
    cams = list(cams())
    lo, h, cells = MO.make_grid(*bounds, res)
    trunc = np.float32(tv * float(h))
    o = TO.fuse(lo, h, cells, cams, trunc, ZNEAR, np.inf, min_obs)
    return SimpleNamespace(name=name, bounds=bounds, resolution=res, cams=cams, trunc_voxels=tv, min_observations=min_obs,
                           lo=lo, h=h, cells=cells, trunc=trunc, **o)


def active_bricks(c):
    """What the sparse grid must at least list: the bricks that hold a cell with a corner some camera observed from
    behind (t < 0)."""
    neg = c.negative
    nz, ny, nx = (s - 1 for s in neg.shape)
    cellmask = np.zeros((nz, ny, nx), dtype=bool)
    for k in range(8):
        cellmask |= neg[(k >> 2):(k >> 2) + nz, ((k >> 1) & 1):((k >> 1) & 1) + ny, (k & 1):(k & 1) + nx]
    return TO.brick_of_cells(cellmask)


def torch_inputs(c, dev):
    """(cameras, depths) for tinysplat_amd.fusion on ``dev``."""
    import torch
    cams = [SimpleNamespace(view_matrix=torch.from_numpy(k["view"].copy()), proj_matrix=torch.from_numpy(k["proj"].copy()),
                            width=k["width"], height=k["height"]) for k in c.cams]
    return cams, [torch.from_numpy(k["depth"].copy()).to(dev) for k in c.cams]


def build_host(directory):
    """g++ build of tests/hostmath/tsdf.cpp: the kernels' header compiled for the host"""
    import ctypes
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    so = Path(directory) / "_tsdf.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(root / "tests" / "hostmath" / "tsdf.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    i32, i64, f32, f64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    lib.th_camera_bytes.restype, lib.th_camera_bytes.argtypes = i32, []
    lib.th_pixel.restype, lib.th_pixel.argtypes = i64, [ptr, f32, f32, f32, f32, ctypes.POINTER(f32)]
    lib.th_observe.restype, lib.th_observe.argtypes = i32, [f32, f32, f32, f32, ctypes.POINTER(f32)]
    lib.th_cull.restype, lib.th_cull.argtypes = i32, [ptr, f32, f32, f32, f32, f32]
    lib.th_unproject.restype, lib.th_unproject.argtypes = i32, [ptr, f64, f64, f64, ctypes.POINTER(f64)]
    return lib
