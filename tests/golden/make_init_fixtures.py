#!/usr/bin/env python
"""Generates tests/golden/init_*.npz by running the REFERENCE's own ``GaussianModel.from_pcd``
(tinysplat/splatting/model_gaussian.py:66-90) on the CPU.

Runs only in the build container (needs the reference checkout).  The real ``sklearn.neighbors`` is
imported before ``make_fixtures.load_reference()``, which stubs only modules that are not loaded yet, so
the nearest-neighbour search is sklearn's own.  ``torch.manual_seed(seed)`` right before the call fixes
the uniforms of ``random_quat_tensor``.  Stored: the inputs (xyz, colours, seed, SH degree), the six
output tensors, ``active_sh_degree`` and the float32 mean neighbour distance behind the scales
(``np.mean(distances[:, 1:], axis=1).astype(np.float32)``, :80, from the same sklearn call).
"""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch
import torch._dynamo  # noqa: F401
import sklearn.neighbors  # noqa: F401  (the real one: load_reference() must not stub it)

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True
import make_fixtures  # noqa: E402
from make_densify_fixtures import KW  # noqa: E402


def surface_cloud(n, seed, outliers=20, dup_block=11):
    """A wavy height-field surface (SfM clouds are surfaces) with far outliers and a block of coincident points."""
    g = np.random.default_rng(seed)
    m = n - outliers - dup_block
    uv = g.uniform(-1.0, 1.0, size=(m, 2))
    z = 0.15 * np.sin(3.0 * uv[:, 0]) * np.cos(2.0 * uv[:, 1])
    pts = [np.stack([uv[:, 0], uv[:, 1], z], axis=1)]
    if outliers:
        d = g.normal(size=(outliers, 3))
        pts.append(d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(20.0, 60.0, size=(outliers, 1)))
    if dup_block:
        pts.append(np.repeat(g.uniform(-0.5, 0.5, size=(1, 3)), dup_block, axis=0))
    xyz = np.concatenate(pts, axis=0)
    return xyz[g.permutation(n)]


def make(mg, name, xyz, seed, sh_degree=3):
    from sklearn.neighbors import NearestNeighbors
    n = xyz.shape[0]
    colors = np.random.default_rng(seed + 1).integers(0, 256, size=(n, 3), dtype=np.uint8)
    pcd = mg.PointCloud(torch.arange(n), torch.as_tensor(xyz), torch.as_tensor(colors), torch.zeros(n))
    torch.manual_seed(seed)
    model = mg.GaussianModel.from_pcd(pcd, device=torch.device("cpu"), **dict(KW, sh_degree=sh_degree))
    dist, _ = NearestNeighbors(n_neighbors=4).fit(xyz).kneighbors(xyz)
    out = {"xyz": xyz, "colors": colors, "seed": seed, "sh_degree": sh_degree,
           "active_sh_degree": model.active_sh_degree, "max_sh_degree": model.max_sh_degree,
           "mean_dist": np.mean(dist[:, 1:], axis=1).astype(np.float32)}
    for f in ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities"):
        out[f] = getattr(model, f).detach().numpy()
    np.savez_compressed(HERE / f"init_{name}.npz", **out)
    print(name, n, xyz.dtype, "-inf scales:", int(np.isinf(out["scales"][:, 0]).sum()))


def main():
    make_fixtures.load_reference()
    mg = importlib.import_module("tinysplat.splatting.model_gaussian")
    mg.PointCloud = importlib.import_module("tinysplat.scene").PointCloud
    make(mg, "n600", surface_cloud(600, 5).astype(np.float32), seed=5)
    make(mg, "n4", np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], dtype=np.float32), seed=6, sh_degree=1)
    make(mg, "n300_f64", surface_cloud(300, 7, outliers=5, dup_block=0), seed=7)


if __name__ == "__main__":
    main()
