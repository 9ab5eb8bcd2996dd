#!/usr/bin/env python
"""Times the SuGaR density regulariser (tinysplat_amd.surface) with device events after a warm-up, and the training
step on the config-3 scene (1 M Gaussians, SH 3, 1920 x 1080, RGB + depth targets) with it on; prints one JSON line
per measurement (ms per call).

  * ``sample_points``: an update step's extra work (sample, k = 16 search, inverse list), M points;
  * ``density_loss + backward``: a non-update active step's term through autograd (both projections);
  * ``TrainStep off (two-launch Adam)`` / ``TrainStep density on`` / ``TrainStep density on, update``: the step
    without the term, on a non-update active step, and on an update step (sampling included).

    python tools/time_density.py [--n 1000000] [--m 100000] [--reps 20] [--out time_density.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd.surface import SurfaceConfig, SurfaceRegularizer, density_loss, sample_points  # noqa: E402
from tinysplat_amd.synthetic import make_scene  # noqa: E402
from tinysplat_amd.training import TrainStep  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    rows = []

    def emit(call, ms, **kw):
        rows.append({"call": call, "ms": round(ms, 4), **kw})
        print(json.dumps(rows[-1]), flush=True)

    w, h = 1920, 1080
    g = torch.Generator().manual_seed(1)
    tgt = torch.rand(h, w, 3, generator=g).to(DEV)
    tgt_d = (2 + 8 * torch.rand(h, w, generator=g)).to(DEV)
    model, cam = make_scene(args.n, 3, w, h)
    model = model.to(DEV)
    model.requires_grad_(True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for weights in ("reference", "area"):
        emit("sample_points", timed(lambda: sample_points(model, args.m, weights, gen), args.reps), n=args.n,
             m=args.m, weights=weights)
    samples = sample_points(model, args.m, "reference", gen)
    depth = tgt_d.clone().requires_grad_(True)
    for projection in ("reference", "screen"):
        def fwd_bwd():
            for p in (model.means, model.scales, model.quats, model.opacities, depth):
                p.grad = None
            density_loss(model, samples, depth, cam, projection).backward()
        emit("density_loss + backward", timed(fwd_bwd, args.reps), n=args.n, m=args.m, projection=projection)
    del model, samples
    torch.cuda.empty_cache()

    for label, cfg, step_no in (
            ("TrainStep off (two-launch Adam)", None, 2),
            ("TrainStep density on", SurfaceConfig(regularize_density=True, regularize_density_start=1,
                                                   regularize_density_end=1 << 30, density_samples=args.m,
                                                   density_projection="screen"), 2),
            ("TrainStep density on, update", SurfaceConfig(regularize_density=True, regularize_density_start=1,
                                                           regularize_density_end=1 << 30, density_samples=args.m,
                                                           density_projection="screen", density_interval=2), 3)):
        model, cam = make_scene(args.n, 3, w, h)
        model = model.to(DEV)
        step = TrainStep(model, DEV, fused_adam=cfg is not None)
        surface = SurfaceRegularizer(cfg, torch.Generator(device=DEV).manual_seed(0)) if cfg else None
        if surface is None:
            step.fused_adam = False
        emit(label, timed(lambda: step(cam, tgt, tgt_d, step=step_no, surface=surface), args.reps), n=args.n,
             m=args.m, width=w, height=h)
        del step, model, surface
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
