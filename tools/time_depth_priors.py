#!/usr/bin/env python
"""Times the batched depth-prior pass on a synthetic dataset.

    python tools/time_depth_priors.py --cameras 200 --points 5000 --width 1920 --height 1080

Every camera gets ``--points`` visible SfM points (the scenes of tests/depth_prior_cases.py: collisions, points outside
the image and behind the camera included) and a dense map of its own size.  Timed with the maps already on the device:
``match_scale`` - projection, sort, de-duplication, sampling, the exact fit and the float32 targets of all cameras - and
its parts.  The reference's own per-camera host path for the same sizes is timed by
``tests/golden/make_depth_fixtures.py --timing``; that comparison is GPU against host.
"""
import argparse
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cameras", type=int, default=200)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import depth_prior_cases as DC
    from tinysplat_amd import PointCloud, match_scale
    from tinysplat_amd.depth import _sparse, apply_scale, fit_scale
    dev = args.device
    cases = [DC.scene_case(args.width, args.height, args.points, seed) for seed in range(args.cameras)]
    ids = [c.ids * 1024 + k for k, c in enumerate(cases)]
    pcd = PointCloud(torch.from_numpy(np.concatenate(ids)).to(dev), torch.from_numpy(np.concatenate([c.xyz for c in cases])).to(dev),
                     torch.zeros((args.cameras * args.points, 3), dtype=torch.uint8, device=dev),
                     torch.from_numpy(np.concatenate([c.errors for c in cases])).to(dev))
    cams = [SimpleNamespace(view_matrix=torch.from_numpy(c.view.copy()), f_x=c.f_x, f_y=c.f_y, width=c.width, height=c.height,
                            visible_point_ids=torch.from_numpy(i).to(dev), name=c.name) for c, i in zip(cases, ids)]
    maps = [torch.from_numpy(c.dense.copy()).to(dev) for c in cases]

    def timed(fn):
        times, out = [], None
        for _ in range(args.repeats + 1):                      # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times[1:]), out
    total, (fits, targets) = timed(lambda: match_scale(maps, cams, pcd))
    del targets
    t_sparse, sparse = timed(lambda: _sparse(cams, pcd, maps))
    t_fit, table = timed(lambda: fit_scale(sparse.x, sparse.z, sparse.weight, sparse.offsets))
    t_apply, _ = timed(lambda: [apply_scale(d, table[i], args.height, args.width) for i, d in enumerate(maps)])
    print(f"{args.cameras} cameras x {args.points} visible points at {args.width}x{args.height}, "
          f"{int(fits[:, 3].sum())} survivors, best of {args.repeats}:")
    print(f"  match_scale (all of it)            {total * 1e3:9.2f} ms")
    print(f"  project + sort + de-duplicate      {t_sparse * 1e3:9.2f} ms")
    print(f"  fit ({int(fits[:, 4].max())} evaluations at most)      {t_fit * 1e3:9.2f} ms")
    print(f"  targets ({args.cameras} launches)             {t_apply * 1e3:9.2f} ms")


if __name__ == "__main__":
    main()
