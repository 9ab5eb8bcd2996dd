#!/usr/bin/env python
"""Generates tests/golden/depth_prior.npz from the REFERENCE's own code (tinysplat/depth.py:73-145).

    python tests/golden/make_depth_fixtures.py --reference <checkout of the reference> [--timing CAMERAS POINTS]

Runs only where the reference's checkout is (nothing here ships anywhere but the .npz data it writes).  The module
``tinysplat/depth.py`` is loaded by itself, with an empty stub for ``cv2`` in ``sys.modules`` (nothing on the two paths
driven here uses it) and the real scipy; ``DepthEstimator`` is constructed with ``skip_init=True`` on an empty scene, so no
network is loaded, and its ``_estimate_sparse`` and ``_match_scale`` run unmodified on the CPU.  ``_match_scale`` returns
the scaled map, not the fit, so the module's ``minimize`` is wrapped to keep scipy's result.

The scene: one 64 x 48 camera, neither at the origin nor axis-aligned, and 220 visible points made by back-projecting
pixel positions - among them collisions (several points on one pixel: the last in the list must win) and points outside
the image.  No point lies behind the camera and every error is positive, so the reference's lists are aligned.  No
projected coordinate, in float64, lies within 1e-3 px of a rounding boundary (asserted): float32 summation order cannot
move a pixel.  The dense map is smooth; the points' depths are 1.6 D + 0.4 plus noise, a fifth of them far off.

Stored: the inputs; the reference's sparse lists (row, col, z, e); its Nelder-Mead ``s, t``, objective value and number of
evaluations.  ``--timing`` instead runs the reference's per-camera host path on a synthetic set of that size and prints
the seconds it takes (DESIGN.md section 6o quotes it beside the batched GPU pass).
"""
import argparse
import importlib.util
import sys
import tempfile
import time
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.dont_write_bytecode = True
import depth_prior_oracle as DO  # noqa: E402

W, H, N = 64, 48, 220


def load_reference(checkout):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_depth", str(Path(checkout) / "tinysplat" / "depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kept = []
    scipy_minimize = mod.minimize

    def minimize(*args, **kwargs):
        kept.append(scipy_minimize(*args, **kwargs))
        return kept[-1]
    mod.minimize = minimize
    mod.tqdm = lambda it, *a, **k: it
    with tempfile.TemporaryDirectory() as tmp:
        est = mod.DepthEstimator(SimpleNamespace(cameras=[]), None, skip_init=True, device="cpu",
                                 depths_path=str(Path(tmp) / "depths"), depth_model=None)
    return est, kept


class Cloud:
    """scene.PointCloud's lookup: points sorted by id, ``get_points`` by searchsorted"""

    def __init__(self, ids, xyz, errors):
        order = np.argsort(ids)
        self.point_ids = torch.from_numpy(ids[order])
        self.xyz, self.errors = torch.from_numpy(xyz[order]), torch.from_numpy(errors[order])

    def get_points(self, ids):
        idx = torch.searchsorted(self.point_ids, ids)
        return self.xyz[idx], None, self.errors[idx]


def camera_of(view, f_x, f_y, width, height, ids):
    return SimpleNamespace(view_matrix=torch.from_numpy(view), f_x=f_x, f_y=f_y, width=width, height=height,
                           visible_point_ids=ids)


def make_scene(rng, width, height, n, outside=0.06):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    rot = np.array([[1 - 2 * (c * c + d * d), 2 * (b * c - a * d), 2 * (b * d + a * c)],
                    [2 * (b * c + a * d), 1 - 2 * (b * b + d * d), 2 * (c * d - a * b)],
                    [2 * (b * d - a * c), 2 * (c * d + a * b), 1 - 2 * (b * b + c * c)]])
    trans = rng.uniform(-1.0, 1.0, 3)
    f_x, f_y = 0.9 * width, 0.85 * width
    yy, xx = np.mgrid[0:height, 0:width]
    dense = (1.5 + 0.8 * np.sin(xx / width * 4.0) * np.cos(yy / height * 3.0) + 0.3 * xx / width).astype(np.float32)
    pu, pv = rng.integers(0, width, n), rng.integers(0, height, n)
    again = rng.random(n) < 0.15                               # collisions: an earlier point's pixel once more
    for i in np.flatnonzero(again)[1:]:
        j = rng.integers(0, i)
        pu[i], pv[i] = pu[j], pv[j]
    z = 1.6 * dense[pv, pu].astype(np.float64) + 0.4 + rng.normal(0.0, 0.02, n)
    z = np.where(rng.random(n) < 0.2, z + rng.uniform(-1.0, 2.0, n), z)
    u, v = pu + rng.uniform(-0.3, 0.3, n), pv + rng.uniform(-0.3, 0.3, n)
    out = rng.random(n) < outside
    u = np.where(out, u + width * rng.choice([-1.0, 1.0], n), u)
    cam = np.stack([(u - width / 2) / f_x * z, (v - height / 2) / f_y * z, z], axis=1)
    xyz = (cam - trans) @ rot
    view = np.eye(4, dtype=np.float64)
    view[:3, :3], view[:3, 3] = rot, trans
    ids = rng.choice(100 * n, n, replace=False).astype(np.int64) + 7
    errors = rng.uniform(0.1, 2.0, n)
    return view.astype(np.float32), float(f_x), float(f_y), dense, xyz, errors, ids


def run_reference(est, kept, view, f_x, f_y, width, height, dense, xyz, errors, ids):
    cam = camera_of(view, f_x, f_y, width, height, ids)
    d_sparse, e_sparse = est._estimate_sparse(cam, SimpleNamespace(pcd=Cloud(ids, xyz, errors)))
    del kept[:]
    est._match_scale(dense, d_sparse, e_sparse)
    return d_sparse, e_sparse, kept[-1]


def timing(est, kept, cameras, points):
    rng = np.random.default_rng(5)
    width, height = 1920, 1080
    scenes = [make_scene(rng, width, height, points, outside=0.0) for _ in range(min(cameras, 4))]
    t0 = time.perf_counter()
    for view, f_x, f_y, dense, xyz, errors, ids in scenes:
        run_reference(est, kept, view, f_x, f_y, width, height, dense, xyz, errors, ids)
    per = (time.perf_counter() - t0) / len(scenes)
    print(f"reference host path (_estimate_sparse + _match_scale, scipy Nelder-Mead, CPU): {per:.3f} s per camera of "
          f"{points} visible points at {width}x{height}, measured on {len(scenes)} cameras; x {cameras} cameras = "
          f"{per * cameras:.1f} s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's checkout")
    ap.add_argument("--timing", type=int, nargs=2, metavar=("CAMERAS", "POINTS"), default=None)
    args = ap.parse_args()
    est, kept = load_reference(args.reference)
    if args.timing:
        return timing(est, kept, *args.timing)
    view, f_x, f_y, dense, xyz, errors, ids = make_scene(np.random.default_rng(20240607), W, H, N)
    clear = DO.boundary_distance(view, f_x, f_y, W, H, xyz.astype(np.float32))
    assert clear > 1e-3, f"a projected coordinate lies {clear} px from a rounding boundary"
    d_sparse, e_sparse, res = run_reference(est, kept, view, f_x, f_y, W, H, dense, xyz, errors, ids)
    assert np.array_equal(d_sparse.row, e_sparse.row) and np.array_equal(d_sparse.col, e_sparse.col)
    row, col = d_sparse.row.astype(np.int64), d_sparse.col.astype(np.int64)
    z, e = np.asarray(d_sparse.data, dtype=np.float64), np.asarray(e_sparse.data, dtype=np.float64)
    assert np.all(z.astype(np.float32) == z), "the reference's depths are float32 values"
    o_row, o_col, o_z, o_e = DO.sparse(view, np.float32(f_x), np.float32(f_y), W, H, xyz.astype(np.float32), errors,
                                       np.float32)
    print(f"{len(row)} survivors of {N} points ({N - len(set(zip(row.tolist(), col.tolist())))} collided or fell outside); "
          f"clearance {clear:.4f} px")
    print("oracle (float32) against the reference: rows/cols equal", np.array_equal(o_row, row) and np.array_equal(o_col, col),
          "| e equal", np.array_equal(o_e, e), "| z equal", np.array_equal(o_z.astype(np.float64), z),
          "| max |dz|", float(np.max(np.abs(o_z.astype(np.float64) - z))) if len(z) == len(o_z) else None)
    s, t = float(res.x[0]), float(res.x[1])
    x = dense[row, col].astype(np.float64)
    f_ref = float(res.fun)
    print(f"Nelder-Mead: s {s!r} t {t!r} f {f_ref!r} after {res.nfev} evaluations; oracle f at it "
          f"{DO.objective(s, t, x, z, 1.0 / e)!r}; exact optimum {DO.optimum(x, z, 1.0 / e)!r}")
    out = HERE / "depth_prior.npz"
    np.savez_compressed(out, view=view, f_x=f_x, f_y=f_y, width=W, height=H, dense=dense, xyz=xyz, errors=errors, ids=ids,
                        ref_row=row, ref_col=col, ref_z=z, ref_e=e, ref_s=s, ref_t=t, ref_objective=f_ref,
                        ref_nfev=int(res.nfev))
    print(f"wrote {out}: {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
