#!/usr/bin/env python
"""Generates tests/golden/surface_density.npz from the REFERENCE's own code (scripts/train.py:77-105,
tinysplat/splatting/model_gaussian.py:244-326).

Runs only in the build container (needs the reference checkout).  ``make_fixtures.load_reference()`` stubs the
third-party imports; pytorch3d's ``knn_points`` is replaced by an exact brute force ordered by (float64 distance,
index).  The reference's ``GaussianModel`` methods run on float32 CPU tensors with the reference's ``Camera``
matrices.  Stored:
  * the command-line defaults of ``arg_parser()`` for the density term, and ``--interval-densify``;
  * on probe steps: the update rule of train.py:78 and the prune rule of train.py:103;
  * per case: the parameters, ``sample_points``' rows, its normals (``torch.randn_like`` captured while it runs)
    and points, the neighbours, a smooth synthetic depth plane, density / mask / approx / loss, autograd's gradients
    for means, scales, quats, opacities and depth (``loss.backward(retain_graph=True)``), and the gradients of a
    second, non-update step after an in-place parameter change (the frozen sampling graph);
  * a "tiny" case whose extent keeps the reference's unnormalised grid inside the image.
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True
import make_fixtures  # noqa: E402
import make_surface_fixtures  # noqa: E402

PROBE_STEPS = [1, 100, 101, 201, 8999, 9000, 9001, 9002, 9100, 9101, 9201, 14999, 15000, 15001]


def exact_knn(points, means, K):
    d = torch.cdist(points[0].double(), means[0].double(), compute_mode="donot_use_mm_for_euclid_dist")
    return SimpleNamespace(idx=torch.argsort(d, dim=1, stable=True)[:, :K][None])


def reference_model(mg, means, scales, quats, opacities):
    m = mg.GaussianModel.__new__(mg.GaussianModel)
    torch.nn.Module.__init__(m)
    m.device = torch.device("cpu")
    for k, v in (("means", means), ("scales", scales), ("quats", quats), ("opacities", opacities)):
        setattr(m, k, torch.nn.Parameter(torch.as_tensor(v, dtype=torch.float32).clone()))
    return m


def run_case(mg, scene, name, n, m, width, height, extent, seed, out):
    g = torch.Generator().manual_seed(seed)
    means = torch.cat((extent * (2 * torch.rand(n, 2, generator=g) - 1) + extent,
                       1.0 + extent * torch.rand(n, 1, generator=g)), 1)
    scales = torch.log(extent * (0.05 + 0.3 * torch.rand(n, 3, generator=g)))
    quats = torch.randn(n, 4, generator=g)
    opac = 2.0 * torch.randn(n, 1, generator=g)
    model = reference_model(mg, means, scales, quats, opac)
    fov_x = np.radians(60.0)
    f = width / (2.0 * np.tan(fov_x / 2.0))
    fov_y = 2.0 * np.arctan(height / (2.0 * f))
    cam = scene.Camera(position=np.zeros(3), f_x=f, f_y=f, fov_x=fov_x, fov_y=fov_y, quat=np.array([1.0, 0, 0, 0]),
                       near=0.001, far=1000.0, image=torch.zeros(height, width, 3), device="cpu")
    yy, xx = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32),
                            indexing="ij")
    depth = 1.0 + extent * (0.5 + 0.2 * xx / width + 0.2 * yy / height + 0.1 * torch.sin(0.3 * xx) * torch.cos(0.2 * yy))
    depth = depth.clone().requires_grad_(True)
    normals = []
    real = torch.randn_like

    def capture(t, *a, **k):
        r = real(t, *a, **k)
        normals.append(r.clone())
        return r

    torch.manual_seed(seed + 1)
    torch.randn_like = capture
    try:
        points, idxs = model.sample_points(num_samples=m)
    finally:
        torch.randn_like = real
    p = {"means": model.means, "scales": model.scales, "quats": model.quats, "opacities": model.opacities}
    pre = {k: v.detach().clone().numpy() for k, v in p.items()}
    # step 1: an update step (train.py:80-91)
    density, nbr = model.density_function(points, update_neighbors=True)
    beta = torch.exp(model.scales).min(dim=-1)[0][nbr].mean(dim=1)
    approx, mask = model.approximate_density_function(points, depth, cam, beta)
    loss = (density[mask] - approx).abs().mean()
    loss.backward(retain_graph=True)
    c = f"{name}_"
    out.update({c + "width": np.array(width), c + "height": np.array(height),
                c + "view_matrix": cam.view_matrix.numpy(), c + "proj_matrix": cam.proj_matrix.numpy(),
                c + "depth": depth.detach().numpy(), c + "rows": idxs.numpy(), c + "normals": normals[0].numpy(),
                c + "points": points.detach().numpy(), c + "knn": nbr.numpy(), c + "density": density.detach().numpy(),
                c + "mask": mask.numpy(), c + "approx": approx.detach().numpy(), c + "loss": loss.detach().numpy(),
                c + "grad_depth": depth.grad.numpy()})
    for k, v in p.items():
        out[c + k] = pre[k]
        out[c + "grad_" + k] = v.grad.numpy().copy()
        v.grad = None
    depth.grad = None
    # step 2: no update - the parameters move in place, the points and their graph stay (train.py:81, :94)
    with torch.no_grad():
        for k, v in p.items():
            v.add_(0.01 * torch.randn(v.shape, generator=g))
    density, nbr = model.density_function(points, update_neighbors=False)
    beta = torch.exp(model.scales).min(dim=-1)[0][nbr].mean(dim=1)
    approx, mask = model.approximate_density_function(points, depth, cam, beta)
    loss = (density[mask] - approx).abs().mean()
    loss.backward(retain_graph=True)
    out[c + "step2_loss"] = loss.detach().numpy()
    out[c + "step2_mask"] = mask.numpy()
    out[c + "step2_grad_depth"] = depth.grad.numpy()
    for k, v in p.items():
        out[c + "step2_" + k] = v.detach().numpy().copy()
        out[c + "step2_grad_" + k] = v.grad.numpy().copy()
    print(name, "mask", int(mask.sum()), "of", m, "loss", float(loss))


def main():
    mod = make_surface_fixtures.load_train_script()
    scene = sys.modules["tinysplat.scene"]
    import importlib
    mg = importlib.import_module("tinysplat.splatting.model_gaussian")
    mg.knn_points = exact_knn
    defaults = mod.arg_parser().parse_args([])
    out = {"default_regularize_density": np.array(bool(defaults.regularize_density)),
           "default_regularize_sdf": np.array(bool(defaults.regularize_sdf))}
    for k in ("lambda_density", "regularize_density_start", "regularize_density_end", "interval_densify"):
        out["default_" + k] = np.array(getattr(defaults, k))
    for flag in (False, True):
        args = mod.arg_parser().parse_args(["--regularize-density"] if flag else [])
        sched = mod.Scheduler(args.regularize_density, args.regularize_density_start, args.regularize_density_end)
        out[f"active_{int(flag)}"] = np.array([bool(sched(s)) for s in PROBE_STEPS])
        out[f"update_{int(flag)}"] = np.array([bool(sched(s)) and (s == sched.start or s % args.interval_densify == 1)
                                              for s in PROBE_STEPS])
        out[f"prune_{int(flag)}"] = np.array([sched.start == s for s in PROBE_STEPS])
    out["probe_steps"] = np.array(PROBE_STEPS)
    run_case(mg, scene, "wide", 500, 256, 64, 48, 1.0, 11, out)
    run_case(mg, scene, "tiny", 400, 256, 64, 48, 0.004, 12, out)
    np.savez_compressed(HERE / "surface_density.npz", **out)


if __name__ == "__main__":
    main()
