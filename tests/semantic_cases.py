"""Scenes, label maps and helpers shared by tests/test_semantic_cpu.py and tests/test_gpu_semantic.py.

A scene is a handful of isotropic Gaussians placed by PIXEL: `place` turns (pixel x, pixel y, depth, sigma in pixels)
into the world position and log-scale that project there for the camera of `camera(w, h)` (at the origin, looking down
+z, principal point at the image centre).  Every GPU case is N <= 200 Gaussians on an image of a few tiles.
"""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import torch

from tinysplat_amd.synthetic import PinholeCamera, SplatModel

import semantic_oracle as SO

ROOT = Path(__file__).resolve().parent.parent
I64P, U8P, F32P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float)


def build_host(directory):
    """g++ build of tests/hostmath/votes.cpp: the kernels' header compiled for the host."""
    so = Path(directory) / "_votes.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    str(ROOT / "tests" / "hostmath" / "votes.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.vh_quantise.restype, lib.vh_quantise.argtypes = ctypes.c_uint32, [ctypes.c_float]
    lib.vh_votes_labels.restype = ctypes.c_int
    lib.vh_votes_labels.argtypes = [ctypes.c_int, ctypes.c_int, I64P, ctypes.c_double, U8P, F32P, I64P, I64P]
    return lib


def host_labels(lib, votes, min_share):
    votes = np.ascontiguousarray(votes, dtype=np.int64)
    n, c = votes.shape
    labels, conf = np.zeros(n, np.uint8), np.zeros(n, np.float32)
    top, total = np.zeros(n, np.int64), np.zeros(n, np.int64)
    assert lib.vh_votes_labels(n, c, votes.ctypes.data_as(I64P), float(min_share), labels.ctypes.data_as(U8P),
                               conf.ctypes.data_as(F32P), top.ctypes.data_as(I64P), total.ctypes.data_as(I64P)) == 0
    return labels, conf, top, total


# ------------------------------------------------------------------------------------------------- rows of votes
def vote_rows():
    """(votes int64 [n, 4], min_share): first-max argmax, ties built on purpose, the min_share edge with
    top == min_share * total exactly (0.25 * 8 and one vote less), all-zero rows, and sums beyond 2^32."""
    rows = np.array([
        [5, 1, 2, 0],              # plain
        [3, 7, 7, 1],              # a tie of two: the smaller column (1)
        [4, 4, 4, 4],              # a tie of all: column 0
        [0, 0, 0, 9],              # the last column alone
        [0, 0, 0, 0],              # empty: 255, confidence 0
        [2, 2, 2, 2],              # top = 2 = 0.25 * 8: kept at min_share = 0.25 (>=)
        [2, 2, 2, 3],              # top 3 of 9: share 1/3
        [1, 3, 2, 2],              # top 3 of 8 = 0.375
        [1 << 40, (1 << 40) + 1, 0, 5],      # beyond 32 bits
        [0, 1, 0, 0],
    ], dtype=np.int64)
    return rows


MIN_SHARES = (0.0, 0.25, 0.375, 0.5, 1.0)


# ------------------------------------------------------------------------------------------------------- scenes
def camera(w, h, name=None):
    cam = PinholeCamera.look_at_origin_plus_z(w, h)
    if name is not None:
        cam.name = name
    return cam


def place(cam, px, py, z, sigma_px, logit, seed=0):
    """Gaussians centred on pixel coordinates (px, py) (sample positions: pixel i covers [i, i + 1)) at depths z with an
    isotropic extent of sigma_px pixels and opacity logits `logit` -> SplatModel on the CPU (SH degree 0)."""
    px, py, z, sigma_px, logit = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (px, py, z, sigma_px, logit))
    n = max(len(a) for a in (px, py, z, sigma_px, logit))
    px, py, z, sigma_px, logit = (np.broadcast_to(a, (n,)).copy() for a in (px, py, z, sigma_px, logit))
    x = (px - cam.width / 2) / cam.f_x * z
    y = (py - cam.height / 2) / cam.f_y * z
    means = torch.tensor(np.stack([x, y, z], axis=1), dtype=torch.float32)
    scales = torch.tensor(np.log(np.abs(sigma_px * z / cam.f_x) + 1e-12), dtype=torch.float32)[:, None].repeat(1, 3)
    quats = torch.zeros((n, 4), dtype=torch.float32)
    quats[:, 0] = 1.0
    g = torch.Generator().manual_seed(seed)
    return SplatModel(means, torch.randn((n, 3), generator=g), torch.zeros((n, 0, 3)), scales, quats,
                      torch.tensor(logit, dtype=torch.float32)[:, None], 0, background=torch.zeros(3))


def random_scene(cam, n, seed, sigma=(1.0, 7.0), logit=(-2.0, 3.0)):
    """n Gaussians at random pixels (a tenth of them off the image), depths 2 .. 10, a spread of sizes and opacities."""
    r = np.random.default_rng(seed)
    return place(cam, r.uniform(-0.05 * cam.width, 1.05 * cam.width, n), r.uniform(-0.05 * cam.height, 1.05 * cam.height, n),
                 r.uniform(2.0, 10.0, n), r.uniform(*sigma, n), r.uniform(*logit, n), seed)


def blocky_map(h, w, labels, block, seed, ignore_share=0.0):
    """uint8 [h, w]: every block x block square draws one of `labels` (or, with probability ignore_share, 255)."""
    r = np.random.default_rng(seed)
    by, bx = -(-h // block), -(-w // block)
    coarse = r.choice(np.asarray(labels, dtype=np.uint8), size=(by, bx))
    coarse = np.where(r.random((by, bx)) < ignore_share, np.uint8(255), coarse)
    return np.ascontiguousarray(np.kron(coarse, np.ones((block, block), np.uint8))[:h, :w])


def identity_map(num_classes):
    m = np.full(256, 255, np.uint8)
    m[:num_classes] = np.arange(num_classes, dtype=np.uint8)
    return m


def staging_scene():
    """96 x 16: six tiles in a row whose lists hold 0, 1, 64, 65, 130 and 0 entries.  Tile 3's 65 Gaussians sit on the
    border to tile 4 and are listed in both; tile 4 has 65 of its own.  Faint (alpha 0.02), so that nothing stops."""
    cam = camera(96, 16)
    r = np.random.default_rng(11)
    px = np.concatenate([[24.0], 40 + r.uniform(-2, 2, 64), 64 + r.uniform(-0.4, 0.4, 65), 72 + r.uniform(-2, 2, 65)])
    py = 8 + r.uniform(-2, 2, len(px))
    return cam, place(cam, px, py, r.uniform(2, 10, len(px)), 1.0, math.log(0.02 / 0.98), 11), [0, 1, 64, 65, 130, 0]


def opaque_stack():
    """32 x 32, twelve screen-filling Gaussians of alpha 0.98 in depth order, in front of a faint one: a pixel stops at
    the third of them at the latest."""
    cam = camera(32, 32)
    z = np.concatenate([np.linspace(2.0, 4.0, 12), [6.0]])
    return cam, place(cam, 16.0, 16.0, z, 40.0, np.concatenate([np.full(12, math.log(0.98 / 0.02)), [-1.0]]), 5)


def clusters_scene(cam, grid=(2, 1), per_cluster=60, seed=3):
    """grid[0] x grid[1] well-separated clusters, one per cell of the image (each fills the middle 40 % of its cell, at a
    depth of its own) -> (model, labels uint8 [N]: the cluster's number)."""
    r = np.random.default_rng(seed)
    gx, gy = grid
    cw, ch = cam.width / gx, cam.height / gy
    px, py, z = [], [], []
    for j in range(gy):
        for i in range(gx):
            px.append((i + r.uniform(0.3, 0.7, per_cluster)) * cw)
            py.append((j + r.uniform(0.3, 0.7, per_cluster)) * ch)
            z.append(r.uniform(3.0, 3.5, per_cluster) + (j * gx + i))
    n = gx * gy * per_cluster
    model = place(cam, np.concatenate(px), np.concatenate(py), np.concatenate(z), r.uniform(1.0, 1.8, n),
                  r.uniform(-1.5, 0.5, n), seed)
    return model, np.repeat(np.arange(gx * gy, dtype=np.uint8), per_cluster)


def mixed_scene():
    """50 x 37 (ragged right and bottom tiles), 150 random Gaussians and, behind them in the tensors: [150] one faint
    Gaussian in front that covers every tile, [151:153] two on the GENERAL path whose 0.999 clamp bites (opacity 0.99988,
    centred on a pixel's sample position, so alpha > 0.999 there), [153:155] two behind the camera, [155] one far outside
    the image (radius 0 / no tiles)."""
    cam = camera(50, 37)
    base = random_scene(cam, 150, 21)
    extra = place(cam, [25.0, 12.5, 40.5, 20.0, 30.0, -4000.0], [18.0, 9.5, 30.5, 10.0, 20.0, 18.0],
                  [1.5, 1.8, 1.9, -3.0, -5.0, 5.0], [200.0, 5.0, 4.0, 5.0, 5.0, 2.0], [-1.0, 9.0, 9.0, 2.0, 2.0, 2.0], 22)
    both = [torch.cat([a, b]) for a, b in zip(base.parameters(), extra.parameters())]
    return cam, SplatModel(*both, active_sh_degree=0, background=torch.zeros(3))


# -------------------------------------------------------------------------------------------------- GPU helpers
def project(model, cam):
    from tinysplat_amd import ops
    from tinysplat_amd.rasterizer import project_args
    return ops.project_gaussians(*project_args(model, cam, (cam.width, cam.height), model.means.device))[:5]


def weight_table(model, cam):
    """The exact reference: float32 [N, H, W] numpy, table[g, p] = vis_g(p), harvested from the existing forward with
    one-hot colours, four Gaussians per pass -> (table, radii int32 numpy)."""
    from tinysplat_amd import ops
    dev = model.means.device
    n, w, h = model.means.shape[0], cam.width, cam.height
    with torch.no_grad():
        xys, depths, radii, conics, nth = project(model, cam)
        table = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
        background = torch.zeros(4, device=dev)
        for at in range(0, n, 4):
            one_hot = torch.zeros((n, 4), device=dev)
            for j in range(min(4, n - at)):
                one_hot[at + j, j] = 1.0
            img, _ = ops.rasterize_gaussians(xys, depths, radii, conics, nth, one_hot, model.opacities, h, w, background,
                                             logit_opacity=True)
            table[at:at + 4] = img.permute(2, 0, 1)[:min(4, n - at)]
    return table.cpu().numpy(), radii.cpu().numpy()


def lists_and_final_T(model, cam):
    """-> (list length per 16x16 tile int [tiles], final_T float32 [H, W] numpy) of the forward launch on the scene."""
    from tinysplat_amd import _lib, ops
    from tinysplat_amd.ops import _call, _ptr, _stream
    dev = model.means.device
    n, w, h = model.means.shape[0], cam.width, cam.height
    with torch.no_grad():
        xys, depths, radii, conics, nth = project(model, cam)
        b = ops.bin_gaussians(xys, depths, radii, nth, h, w, use_cache=False)
        bins = b.tile_bins.cpu().numpy()
        final_T = torch.ones((h, w), device=dev)
        if b.num_intersects:
            splats = torch.empty((n, 12), device=dev)
            out = torch.empty((h, w, 3), device=dev)
            fidx = torch.empty((h, w), dtype=torch.int32, device=dev)
            zeros = torch.zeros((n, 3), device=dev)
            lib, s = _lib.load(), _stream(dev)
            _call("ts_pack_splats", lib.ts_pack_splats, n, 3, 1, _ptr(xys), _ptr(radii), _ptr(conics), _ptr(zeros),
                  _ptr(model.opacities.contiguous()), _ptr(b.cum_tiles_hit), b.cam, None, _ptr(splats), s)
            _call("ts_raster_fwd", lib.ts_raster_fwd, 3, 0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted),
                  _ptr(splats), _ptr(zeros), _ptr(out), _ptr(final_T), _ptr(fidx), None, s)
    return bins[:, 1] - bins[:, 0], final_T.cpu().numpy()


def expected_votes(table, label_map, class_map, num_classes):
    col = None if label_map is None else SO.columns(label_map, class_map, num_classes)
    return SO.votes_from_table(table, col, num_classes)
