#!/usr/bin/env python
"""Times the appearance stage: the forward, the backward with its sum launch and the optimiser step
on one image with ``ops.kernel_timer``, each entry's share of its own byte count at a streaming rate, and a full
``TrainStep`` with and without an ``AppearanceModel`` on BASELINE configs[2] (1M Gaussians, SH 3, 1920x1080).

    python tools/time_appearance.py --json profiles/appearance_times.json

Prints one JSON object.  Needs a GPU."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, nargs=3, default=[8, 16, 16], metavar=("L", "H", "W"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--gaussians", type=int, default=1_000_000, help="of the TrainStep comparison; 0 skips it")
    ap.add_argument("--steps", type=int, default=30, help="timed steps of each TrainStep run, interleaved in blocks of 10")
    ap.add_argument("--stream-tbps", type=float, default=5.0, help="the streaming rate the byte counts are held against")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def time_entries(args):
    import torch
    from tinysplat_amd.appearance import AppearanceConfig, AppearanceModel
    from tinysplat_amd.ops import kernel_timer
    h, w, dev = args.height, args.width, "cuda:0"
    model = AppearanceModel(1, AppearanceConfig(grid=tuple(args.grid)), dev)
    g = torch.Generator().manual_seed(0)
    model.grids += (0.05 * torch.randn(model.grids.shape, generator=g)).to(dev)
    image = torch.rand(h, w, 3, generator=g).to(dev).requires_grad_(True)
    v_out = torch.randn(h, w, 3, generator=g).to(dev)
    for timed in (False, True):                          # one warm-up round, then the timed one
        if timed:
            kernel_timer.start()
        for _ in range(args.repeats if timed else 5):
            image.grad = None
            model.apply(image, 0).backward(v_out)
            model.step(0)
    times = kernel_timer.stop()
    image_bytes, grid_bytes = h * w * 12, model.grids[0].numel() * 4
    moved = {"ts_appearance_fwd": 2 * image_bytes, "ts_appearance_bwd": 3 * image_bytes,
             "ts_grid_tv": 3 * grid_bytes, "ts_adam_step": 7 * grid_bytes}
    out = {}
    for name, nbytes in moved.items():
        launches, ms = times[name]
        floor_us = nbytes / (args.stream_tbps * 1e12) * 1e6
        out[name] = {"launches": launches, "mean_us": ms * 1e3, "bytes": nbytes, "streaming_floor_us": floor_us,
                     "fraction_of_streaming_rate": floor_us / (ms * 1e3)}
    return out


def time_train_step(args):
    import torch
    from tinysplat_amd.appearance import AppearanceConfig, AppearanceModel
    from tinysplat_amd.synthetic import make_scene
    from tinysplat_amd.training import TrainStep
    h, w, dev = args.height, args.width, "cuda:0"
    target = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    runs = {}
    for name in ("without", "with"):
        model, cam = make_scene(args.gaussians, 3, w, h, seed=0)
        model = model.to(dev)
        appearance = AppearanceModel(1, AppearanceConfig(grid=tuple(args.grid)), dev) if name == "with" else None
        runs[name] = (TrainStep(model, dev), cam, dict(appearance=appearance, view=0) if appearance else {})
    for step, cam, extra in runs.values():               # warm-up
        for _ in range(5):
            step(cam, target, **extra)
    samples = {name: [] for name in runs}
    for _block in range(max(1, args.steps // 10)):       # interleaved blocks: drift hits both runs alike
        for name, (step, cam, extra) in runs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                step(cam, target, **extra)
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / 10.0)
    return {name: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v),
                   "blocks_of_10": len(v)} for name, v in samples.items()}


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    result = {"image": [args.height, args.width], "grid": list(args.grid), "stream_tbps": args.stream_tbps,
              "device": torch.cuda.get_device_name(0), "entries": time_entries(args)}
    if args.gaussians > 0:
        result["train_step"] = dict(time_train_step(args), gaussians=args.gaussians)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
