#!/usr/bin/env python
"""Times the antialiased mode: ``ts_antialias_fwd`` and ``ts_antialias_bwd`` on the Gaussians of
the BASELINE configs[2] frame (1M Gaussians, SH 3, 1920x1080) - the forward launch as the frame issues it (o_eff and the
records) and as the stand-alone op issues it (comp alone), the backward launch on the radii of that frame's projection -
each against ``ts_bench_stream_read`` over as many bytes as the launch reads and writes, with device events, interleaved
in blocks after untimed warm-up launches.  Then ``TrainStep`` on that frame in both modes, fused Adam on, and the frame's
listed (Gaussian, tile) pairs in both modes.

    python tools/time_antialias.py --json profiles/antialias_times.json

Prints one JSON object.  Needs a GPU."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FWD_BYTES = 44 + 20          # means 12, scales 12, quats 16, logit 4 read; o_eff 4 and the record 16 written
FWD_COMP_BYTES = 40 + 4      # the stand-alone op: no opacity read, comp written
BWD_BYTES = 40 + 16          # radii 4, record 16, logit 4, v_opacity 4, v_conic 12 read; v_opacity 4, v_conic 12 written


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per variant, interleaved")
    ap.add_argument("--repeats", type=int, default=20, help="launches per block")
    ap.add_argument("--steps", type=int, default=60, help="timed steps of each TrainStep run, in blocks of 10; 0 skips them")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def timed(variants, blocks, repeats):
    import torch
    for fn in variants.values():                                       # warm-up, untimed
        for _ in range(3):
            fn()
    samples = {name: [] for name in variants}
    for _block in range(blocks):                                       # interleaved blocks: drift hits every variant alike
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeats):
                fn()
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / repeats * 1e3)
    return samples


def time_kernels(args):
    import torch
    from tinysplat_amd import _lib, frame, ops
    from tinysplat_amd.ops import _ptr, _stream
    from tinysplat_amd.rasterizer import camera_on_device, tile_bounds
    from tinysplat_amd.synthetic import make_scene
    dev = torch.device("cuda:0")
    lib = _lib.load()
    model, cam = make_scene(args.gaussians, 3, args.width, args.height, seed=0)
    model = model.to(dev)
    n, w, h = int(model.means.shape[0]), args.width, args.height
    view, projview, origin = camera_on_device(cam, dev)
    view34 = view[:3, :].contiguous()
    tscam = ops._camera(cam.f_x, cam.f_y, w / 2, h / 2, h, w, tile_bounds((w, h)))
    f32 = dict(dtype=torch.float32, device=dev)
    comp, o_eff, rows = torch.empty((n,), **f32), torch.empty((n,), **f32), torch.empty((n, 4), **f32)
    logits = model.opacities.detach().contiguous()
    pairs = {}
    with torch.no_grad():
        for mode in ("classic", "antialiased"):
            model.rasterize_mode = mode
            _, _, _, radii = frame.render_frame_planes(model, view34, projview, origin, cam.f_x, cam.f_y, w, h)
            b = frame.last_binning[0]
            pairs[mode] = {"bounding_box_pairs": int(b.num_intersects),
                           "listed_pairs": int((b.tile_bins[:, 1] - b.tile_bins[:, 0]).sum())}
    radii = radii.clone()
    gen = torch.Generator().manual_seed(3)
    v_opacity, v_conic = torch.randn(n, generator=gen).to(dev), torch.randn(n, 3, generator=gen).to(dev)
    sink = torch.zeros((1,), **f32)
    flats = {k: torch.empty((k * n // 4,), **f32).normal_() for k in sorted({FWD_BYTES, FWD_COMP_BYTES, BWD_BYTES})}
    s = _stream(dev)

    def fwd():
        _lib.check(lib.ts_antialias_fwd(n, _ptr(model.means), _ptr(model.scales), _ptr(model.quats), _ptr(view34), tscam, 3,
                                        _ptr(logits), _lib.RASTER_LOGIT_OPACITY, None, _ptr(o_eff), _ptr(rows), s),
                   "ts_antialias_fwd")

    def fwd_comp():
        _lib.check(lib.ts_antialias_fwd(n, _ptr(model.means), _ptr(model.scales), _ptr(model.quats), _ptr(view34), tscam, 3,
                                        None, 0, _ptr(comp), None, None, s), "ts_antialias_fwd")

    def bwd():                     # (in place: v_opacity and v_conic drift from launch to launch, the traffic does not)
        _lib.check(lib.ts_antialias_bwd(n, _ptr(radii), _ptr(rows), _ptr(logits), _lib.RASTER_LOGIT_OPACITY,
                                        _ptr(v_opacity), _ptr(v_conic), s), "ts_antialias_bwd")

    def stream_read(nbytes):
        flat = flats[nbytes]
        return lambda: _lib.check(lib.ts_bench_stream_read(_ptr(flat), flat.numel(), _ptr(sink), s), "ts_bench_stream_read")
    fwd()
    variants = {"ts_antialias_fwd": fwd, "stream_read_fwd_bytes": stream_read(FWD_BYTES),
                "ts_antialias_fwd_comp_only": fwd_comp, "stream_read_fwd_comp_bytes": stream_read(FWD_COMP_BYTES),
                "ts_antialias_bwd": bwd, "stream_read_bwd_bytes": stream_read(BWD_BYTES)}
    samples = timed(variants, args.blocks, args.repeats)
    nbytes = {"ts_antialias_fwd": FWD_BYTES, "stream_read_fwd_bytes": FWD_BYTES, "ts_antialias_fwd_comp_only": FWD_COMP_BYTES,
              "stream_read_fwd_comp_bytes": FWD_COMP_BYTES, "ts_antialias_bwd": BWD_BYTES, "stream_read_bwd_bytes": BWD_BYTES}
    out = {"visible_gaussians": int((radii > 0).sum()), "pairs": pairs,
           "compensation": {"mean": float(o_eff.sum() / torch.sigmoid(logits).sum()),
                            "zero": int((rows[:, 3] == 0).sum())}}
    for key, v in samples.items():
        med = statistics.median(v)
        out[key] = {"bytes_per_gaussian": nbytes[key], "us_median": med, "us_min": min(v), "us_max": max(v),
                    "tb_per_s": nbytes[key] * n / med / 1e6}
    for kernel, base in (("ts_antialias_fwd", "stream_read_fwd_bytes"), ("ts_antialias_fwd_comp_only", "stream_read_fwd_comp_bytes"),
                         ("ts_antialias_bwd", "stream_read_bwd_bytes")):
        out[kernel]["fraction_of_stream_read_rate"] = out[base]["us_median"] / out[kernel]["us_median"]
    return out


def time_train_step(args):
    import torch
    from tinysplat_amd.synthetic import make_scene
    from tinysplat_amd.training import TrainStep
    h, w, dev = args.height, args.width, "cuda:0"
    target = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    runs = {}
    for mode in ("classic", "antialiased"):
        model, cam = make_scene(args.gaussians, 3, w, h, seed=0)
        model = model.to(dev)
        model.rasterize_mode = mode
        runs[mode] = (TrainStep(model, dev), cam)
    for step, cam in runs.values():                      # warm-up
        for _ in range(8):
            step(cam, target)
    samples = {name: [] for name in runs}
    for _block in range(max(1, args.steps // 10)):       # interleaved blocks: drift hits every run alike
        for name, (step, cam) in runs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                step(cam, target)
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / 10.0)
    out = {name: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v),
                  "blocks_of_10": len(v), "fused_steps": runs[name][0].optimizer.fused_steps} for name, v in samples.items()}
    out["antialiased_minus_classic_ms"] = out["antialiased"]["ms_per_step_median"] - out["classic"]["ms_per_step_median"]
    return out


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    result = {"gaussians": args.gaussians, "image": [args.height, args.width], "blocks": args.blocks, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "kernels": time_kernels(args)}
    if args.steps > 0:
        result["train_step"] = time_train_step(args)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
