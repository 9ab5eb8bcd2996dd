#!/usr/bin/env python
"""Times the opacity-entropy regulariser (tinysplat_amd.surface) with device events after a warm-up, and the
training step on the config-3 scene (1 M Gaussians, SH 3, 1920 x 1080, RGB + depth targets) with it off and on;
prints one JSON line per measurement (ms per call).

  * ``opacity_entropy``: the C entry alone (value + gradient), N opacities;
  * ``opacity_entropy + backward``: through autograd, as a training step uses it;
  * ``TrainStep off (fused Adam)``: today's step, the update applied inside the frame's backward;
  * ``TrainStep off (two-launch Adam)``: the same step with backward, then one Adam launch;
  * ``TrainStep opacity on``: the step on an active regulariser step (one backward for the whole loss,
    two-launch Adam).

    python tools/time_surface.py [--n 1000000] [--reps 20] [--out time_surface.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd.surface import SurfaceConfig, SurfaceRegularizer, opacity_entropy  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    rows = []

    def emit(call, ms, **kw):
        rows.append({"call": call, "ms": round(ms, 4), **kw})
        print(json.dumps(rows[-1]), flush=True)

    x = (2.0 * torch.randn(args.n, 1, generator=torch.Generator().manual_seed(0))).to(DEV)
    emit("opacity_entropy", timed(lambda: opacity_entropy(x), args.reps), n=args.n)
    xg = x.clone().requires_grad_(True)

    def fwd_bwd():
        xg.grad = None
        opacity_entropy(xg).backward()
    emit("opacity_entropy + backward", timed(fwd_bwd, args.reps), n=args.n)

    w, h = 1920, 1080
    g = torch.Generator().manual_seed(1)
    tgt = torch.rand(h, w, 3, generator=g).to(DEV)
    tgt_d = (2 + 8 * torch.rand(h, w, generator=g)).to(DEV)
    on = SurfaceRegularizer(SurfaceConfig(regularize_opacity=True, regularize_opacity_start=1,
                                          regularize_opacity_end=1 << 30))
    for label, fused, surface in (("TrainStep off (fused Adam)", True, None),
                                  ("TrainStep off (two-launch Adam)", False, None),
                                  ("TrainStep opacity on", True, on)):
        model, cam = make_scene(args.n, 3, w, h)
        model = model.to(DEV)
        step = TrainStep(model, DEV, fused_adam=fused)
        emit(label, timed(lambda: step(cam, tgt, tgt_d, step=1, surface=surface), args.reps), n=args.n, width=w,
             height=h)
        del step, model
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
