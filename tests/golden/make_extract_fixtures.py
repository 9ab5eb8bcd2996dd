#!/usr/bin/env python
"""Generates tests/golden/extract_points.npz from the REFERENCE's own code
(tinysplat/splatting/model_gaussian.py:398-465, tinysplat/scene.py:138-192).

Runs only in the build container (needs the reference checkout).  ``make_fixtures.load_reference()`` stubs the
third-party imports; pytorch3d's ``knn_points`` is replaced by an exact brute force ordered by (float64 distance,
index), ``tqdm`` by the identity, and ``open3d`` by a recorder whose ``Vector3dVector`` captures ``p_intersects`` and
stops the call, so ``extract_mesh_poisson`` runs unmodified up to there.  The ``scene`` handed in returns a stored
depth map; ``density_function``, ``torch.randperm`` and ``Camera.backproject_points`` are wrapped to record the
samples, neighbours, densities, pixel indices and ``p_world``.  The reference runs on float32 CPU tensors (its camera
position is a float64 array, as a dataset gives it, so its ray direction and final sum are promoted to float64).

One model (2000 Gaussians flattened onto a wavy sheet) and three cameras: ``square`` (64 x 64, at the origin),
``wide`` (64 x 48: the pixel quirk) and ``posed`` (48 x 48, neither at the origin nor axis-aligned).  The depth is
the sheet's depth plus noise, with a patch of zero-depth pixels.  Stored per case: the camera, the depth, the pixel
indices and the seed that drew them, ``p_world``, the reference's keep / first decisions and ``p_intersects``; samples and densities of every
16th ray, neighbours of every 64th; ``project_points`` of every 4th intersection; and the measured allowances
(tests/extract_oracle.py is the float64 yardstick, evaluated stage by stage on the reference's own float32 values):
  * ``E_pw``: the largest deviation of the reference's ``p_world`` from the float64 back-projection;
  * ``E_pts`` / ``E_d``: the largest deviation of the reference's ``p_intersects`` / densities from the oracle on
    decision-stable rays, the oracle evaluated on the reference's ``p_world``, samples and neighbours;
  * ``E_n``: the float32 restatement of the oracle's normal against its float64 evaluation at the same points.
The script prints the unstable and kept shares of the reference's own run and refuses to write a fixture with more
than 2 % unstable rays or fewer than half of the rays kept.
"""
import importlib
import inspect
import re
import sys
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.dont_write_bytecode = True
import make_fixtures  # noqa: E402
from make_density_fixtures import reference_model  # noqa: E402
import extract_oracle as EO  # noqa: E402

N = 2000
SAMPLE_STRIDE, KNN_STRIDE = 16, 64
PARAMS = ("means", "scales", "quats", "opacities")


class Captured(Exception):
    def __init__(self, array):
        self.array = array


def stub_modules():
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = tq
    o3d = types.ModuleType("open3d")

    def vector3d(array):
        raise Captured(np.asarray(array))
    o3d.geometry = SimpleNamespace(PointCloud=lambda: SimpleNamespace())
    o3d.utility = SimpleNamespace(Vector3dVector=vector3d)
    sys.modules["open3d"] = o3d


def exact_knn(points, means, K):
    return SimpleNamespace(idx=EO.exact_knn(points[0], means[0], K)[None])


def sheet(x, y):
    return 3.0 + 0.1 * torch.sin(2.0 * x) * torch.cos(1.5 * y)


def make_model(seed):
    g = torch.Generator().manual_seed(seed)
    xy = 2.8 * (2 * torch.rand(N, 2, generator=g) - 1)
    means = torch.cat((xy, sheet(xy[:, 0], xy[:, 1])[:, None] + 0.005 * torch.randn(N, 1, generator=g)), 1)
    scales = torch.log(torch.cat((0.10 + 0.05 * torch.rand(N, 2, generator=g),
                                  0.025 + 0.01 * torch.rand(N, 1, generator=g)), 1))
    quats = torch.cat((torch.ones(N, 1), 0.08 * torch.randn(N, 3, generator=g)), 1)
    opac = 1.5 + 1.0 * torch.randn(N, 1, generator=g)
    return {"means": means, "scales": scales, "quats": quats, "opacities": opac}


def sheet_depth(cam, width, height, position, seed):
    """Camera-space depth of the sheet along every pixel's (screen convention) ray, by fixed-point iteration, plus
    noise, with a patch of zero-depth pixels."""
    g = torch.Generator().manual_seed(seed)
    V = cam.view_matrix.double()
    R = V[:3, :3]
    rows, cols = torch.meshgrid(torch.arange(height, dtype=torch.float64), torch.arange(width, dtype=torch.float64),
                                indexing="ij")
    d_cam = torch.stack(((cols + 0.5 - width / 2) / cam.f_x, (rows + 0.5 - height / 2) / cam.f_y,
                         torch.ones_like(rows)), -1)
    d_world = d_cam @ R                                  # R^T d per pixel
    pos = torch.as_tensor(position, dtype=torch.float64)
    z = torch.full_like(rows, 3.0)
    for _ in range(20):
        w = pos + d_world * z[..., None]
        z = z + (sheet(w[..., 0], w[..., 1]) - w[..., 2]) / d_world[..., 2]
    depth = (z + 0.02 * torch.randn(height, width, generator=g, dtype=torch.float64)).float()
    depth[height // 6:height // 6 + 6, width // 3:width // 3 + 10] = 0.0
    return depth


def run_case(mg, scene, name, params, width, height, position, quat, seed, out):
    model = reference_model(mg, *(params[k] for k in PARAMS))
    fov_x = np.radians(60.0)
    f = width / (2.0 * np.tan(fov_x / 2.0))
    fov_y = 2.0 * np.arctan(height / (2.0 * f))
    position = np.asarray(position, dtype=np.float64)
    cam = scene.Camera(position=position, f_x=f, f_y=f, fov_x=fov_x, fov_y=fov_y, quat=np.asarray(quat, dtype=np.float64),
                       near=0.2, far=20.0, image=torch.zeros(height, width, 3), device="cpu")
    depth = sheet_depth(cam, width, height, position, seed)
    rec = {}
    real_density, real_randperm, real_backproject = mg.GaussianModel.density_function, torch.randperm, \
        scene.Camera.backproject_points

    def density_function(self, points, update_neighbors=True):
        d, nbr = real_density(self, points, update_neighbors)
        rec["samples"], rec["density"], rec["knn"] = points.detach().clone(), d.detach().clone(), nbr.clone()
        return d, nbr

    def randperm(*a, **k):
        rec["idxs"] = real_randperm(*a, **k)
        return rec["idxs"]

    def backproject(self, points, *a, **k):
        rec["p_world"] = real_backproject(self, points, *a, **k)
        return rec["p_world"]

    mg.GaussianModel.density_function, torch.randperm, scene.Camera.backproject_points = density_function, randperm, \
        backproject
    torch.manual_seed(seed)
    try:
        model.extract_mesh_poisson(SimpleNamespace(render=lambda c: (None, {"depth": depth})), [cam])
        raise SystemExit("extract_mesh_poisson did not reach Vector3dVector")
    except Captured as c:
        p_ref = torch.from_numpy(c.array)
    finally:
        mg.GaussianModel.density_function, torch.randperm, scene.Camera.backproject_points = real_density, \
            real_randperm, real_backproject
    ids = rec["idxs"]
    m = ids.shape[0]
    level = 0.3
    d_ref = rec["density"].reshape(m, 21)
    assert d_ref.dtype == torch.float32 and rec["samples"].dtype == torch.float32
    under, above = (d_ref - level) < 0, (d_ref - level) > 0
    first_ref = above.max(dim=-1)[1]
    keep_ref = under[:, 0] & (first_ref != 0)
    assert int(keep_ref.sum()) == p_ref.shape[0]
    # the float64 oracle, stage by stage on the reference's own float32 values (see tests/extract_oracle.py)
    args = (params, depth, cam.view_matrix, cam.proj_matrix, position, ids)
    e2e = EO.level_set_oracle(*args, with_normals=False)
    e_pw = (rec["p_world"].double() - e2e["p_world"])[e2e["valid"]].abs().max().item()
    o = EO.level_set_oracle(*args, given={"p_world": rec["p_world"], "samples": rec["samples"], "knn": rec["knn"]})
    assert torch.equal(EO.exact_knn(rec["samples"][:2100], params["means"]), rec["knn"][:2100])
    stable = o["stable"]
    unstable_share = 1.0 - stable.double().mean().item()
    kept_share = keep_ref.double().mean().item()
    finite = torch.isfinite(d_ref).all(-1)
    # the reference's own float32 run: rays with a sample within DELTA of the level
    margin_ref = torch.where(finite, (d_ref - level).abs().min(-1).values, torch.ones(m))
    print(f"{name}: {m} rays, reference kept {kept_share:.4f}, unstable (reference float32) "
          f"{(margin_ref <= EO.DELTA).double().mean().item():.4f}, unstable (oracle) {unstable_share:.4f}")
    if unstable_share > 0.02 or kept_share < 0.5:
        raise SystemExit(f"{name}: outside the cap (unstable <= 2 %, kept >= 50 %): no fixture written")
    mism = stable & ((keep_ref != o["keep"]) | (keep_ref & (first_ref != o["first"])))
    both = stable & keep_ref & o["keep"] & (first_ref == o["first"])
    p_full = torch.zeros(m, 3, dtype=torch.float64)
    p_full[keep_ref] = p_ref
    e_pts = (p_full - o["points"])[both].abs().max().item()
    rows = stable & o["valid"] & finite
    e_d = (d_ref.double() - o["density"])[rows].abs().max().item()
    # normals: the float32 restatement against the float64 evaluation, at the reference's points
    pts32 = p_ref.float()
    prm = {k: torch.as_tensor(params[k]) for k in PARAMS}
    knn_p = EO.exact_knn(pts32, prm["means"])
    n32 = EO.normals(pts32, knn_p, prm)
    n64 = EO.normals(pts32.double(), knn_p, {k: v.double() for k, v in prm.items()})
    e_n = (n32.double() - n64)[both[keep_ref]].abs().max().item()
    print(f"  keep/first mismatches on stable rays: {int(mism.sum())}; E_pw {e_pw:.3e}  E_pts {e_pts:.3e}  "
          f"E_d {e_d:.3e}  E_n {e_n:.3e}")
    c = name + "_"
    proj_in = p_ref.float()
    out.update({
        c + "width": np.array(width), c + "height": np.array(height), c + "f": np.array(f), c + "seed": np.array(seed),
        c + "position": position, c + "quat": np.asarray(quat, dtype=np.float64),
        c + "view_matrix": cam.view_matrix.numpy(), c + "proj_matrix": cam.proj_matrix.numpy(),
        c + "depth": depth.numpy(), c + "idxs": ids.numpy().astype(np.int32),
        c + "p_world": rec["p_world"].numpy(), c + "keep": keep_ref.numpy(), c + "first": first_ref.numpy().astype(np.int8),
        c + "p_intersects": p_ref.numpy(),
        c + "samples": rec["samples"].reshape(m, 21, 3)[::SAMPLE_STRIDE].numpy(),
        c + "density": d_ref[::SAMPLE_STRIDE].numpy(),
        c + "knn": rec["knn"].reshape(m, 21, 16)[::KNN_STRIDE].numpy().astype(np.int16),
        c + "projected": cam.project_points(proj_in[::4]).numpy(),
        c + "projected_ndc_depth": cam.project_points(proj_in[::4], screen_coordinates=False, return_depth=True).numpy(),
        c + "E_pw": np.array(e_pw), c + "E_pts": np.array(e_pts), c + "E_d": np.array(e_d), c + "E_n": np.array(e_n),
        c + "unstable_share": np.array(unstable_share), c + "kept_share": np.array(kept_share)})


def main():
    stub_modules()
    scene, _, _ = make_fixtures.load_reference()
    mg = importlib.import_module("tinysplat.splatting.model_gaussian")
    mg.knn_points = exact_knn
    src = inspect.getsource(mg.GaussianModel.extract_mesh_poisson)
    lo, hi, steps = re.search(r"torch\.linspace\((-?[\d.]+),\s*(-?[\d.]+),\s*(\d+)\)", src).groups()
    out = {"default_surface_level": np.array(float(re.search(r"surface_level\s*=\s*([\d.]+)", src).group(1))),
           "default_num_total_points": np.array(int(re.search(r"num_total_points\s*=\s*([\d_]+)", src).group(1))),
           "default_num_steps": np.array(int(steps)), "default_extent_sigmas": np.array(float(hi)),
           "default_neighbours": np.array(int(re.search(r"K=(\d+)", src).group(1))),
           "sample_stride": np.array(SAMPLE_STRIDE), "knn_stride": np.array(KNN_STRIDE), "delta": np.array(EO.DELTA)}
    assert float(lo) == -float(hi)
    params = make_model(21)
    for k in PARAMS:
        out[k] = params[k].numpy()
    run_case(mg, scene, "square", params, 64, 64, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 31, out)
    run_case(mg, scene, "wide", params, 64, 48, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 32, out)
    q = np.array([0.985, 0.09, -0.12, 0.07])
    run_case(mg, scene, "posed", params, 48, 48, (0.35, -0.25, -0.4), q / np.linalg.norm(q), 33, out)
    np.savez_compressed(HERE / "extract_points.npz", **out)
    print("wrote", HERE / "extract_points.npz", (HERE / "extract_points.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
