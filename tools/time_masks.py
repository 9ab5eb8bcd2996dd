#!/usr/bin/env python
"""Times the masked loss and the masked metrics with device events after a warm-up and writes
``profiles/mask_times.json``.

Everything runs at BASELINE config 3's size, 1920 x 1080, on the frame as two planes with a depth target, under a random
mask of about 30 % ignored pixels in blobs.  The variants are timed ALTERNATING inside one process, ``--iters`` calls
each, and the whole set is repeated ``--rounds`` times so that the spread of each call is visible beside its median:

  * the unmasked loss pair (``ts_photometric_loss_rgbd`` on a ``ts_loss`` with a depth plane), on this build;
  * the masked loss pair (the same descriptor with ``TS_LOSS_MASKED``);
  * the route a user would otherwise take: the blend as tensor expressions, the unmasked pair, both gradients times m;
  * a streaming read of as many bytes as the masked pair moves (``ts_bench_stream_read``), as the floor;
  * ``image_metrics`` with and without a mask (uint8 target).

    python tools/time_masks.py [--width 1920 --height 1080] [--iters 200] [--rounds 3] [--out profiles/mask_times.json]
                               [--note KEY=VALUE ...]

``--note`` adds a string to the file (the unmasked-path comparison against the parent commit, kernel statistics).
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd import _lib  # noqa: E402
from tinysplat_amd.masks import mask_coverage, mask_weights  # noqa: E402
from tinysplat_amd.metrics import image_metrics  # noqa: E402
from tinysplat_amd.ops import _ptr, _stream  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def blob_mask(h, w, ignored, dev):
    """uint8 [h, w]: smooth noise thresholded so that about ``ignored`` of the pixels are 0, the rest 255."""
    g = torch.Generator().manual_seed(11)
    coarse = torch.rand(1, 1, h // 40 + 2, w // 40 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bicubic", align_corners=False)[0, 0]
    return torch.where(smooth < torch.quantile(smooth.flatten()[::7], ignored), 0, 255).to(torch.uint8).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ignored", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mask_times.json"))
    ap.add_argument("--note", action="append", default=[], metavar="KEY=VALUE")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand(h, w, 3, generator=g)
    tgt = (rgb + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1).to(dev)
    u8 = (tgt * 255.0).round().to(torch.uint8)
    depth = (2.0 + 8.0 * torch.rand(h, w, generator=g)).to(dev)
    dtgt = (2.0 + 8.0 * torch.rand(h, w, generator=g)).to(dev)
    rgb = rgb.to(dev)
    mask = blob_mask(h, w, args.ignored, dev)
    m = mask_weights(mask)
    m3, keep = m[..., None].contiguous(), (mask == 255)[..., None]
    lib = _lib.load()
    ws = torch.empty((int(lib.ts_photometric_ws_floats(h, w)),), dtype=torch.float32, device=dev)
    v_rgb, v_depth = torch.empty_like(rgb), torch.empty_like(depth)
    stream = _stream(dev)
    w_l1, w_ssim, w_depth = 0.8 / (3.0 * h * w), -0.2 / (3.0 * (h - 10) * (w - 10)), 0.2 / (h * w)

    def descriptor(**more):
        return _lib.TsLoss(height=h, width=w, pixel_floats=3, image=_ptr(rgb), depth=_ptr(depth), target=_ptr(tgt),
                           depth_target=_ptr(dtgt), w_l1=w_l1, w_ssim=w_ssim, w_depth=w_depth, ws=_ptr(ws),
                           v_image=_ptr(v_rgb), v_depth=_ptr(v_depth), **more)
    plain, masked = descriptor(), descriptor(flags=_lib.LOSS_MASKED, mask=_ptr(mask))

    def pair(image):
        plain.image = _ptr(image)
        _lib.check(lib.ts_photometric_loss_rgbd(ctypes.byref(plain), stream), "ts_photometric_loss_rgbd")

    def masked_pair():
        _lib.check(lib.ts_photometric_loss_rgbd(ctypes.byref(masked), stream), "ts_photometric_loss_rgbd, masked")

    def torch_route():
        blended = torch.where(keep, rgb, torch.addcmul(tgt, m3, rgb - tgt))
        pair(blended)
        v_rgb.mul_(m3)
        v_depth.mul_(m)

    px, mp = h * w, (h - 10) * (w - 10)
    # the masked pair's own traffic: pass 1 reads image, depth, both targets and the mask and writes nine maps; pass 2 reads
    # them all again and writes both gradients
    moved = 2 * (12 + 4 + 12 + 4 + 1) * px + 2 * 36 * mp + 16 * px
    floor = torch.ones(moved // 4, dtype=torch.float32, device=dev)
    sink = torch.zeros(4, dtype=torch.float32, device=dev)

    def stream_read():
        _lib.check(lib.ts_bench_stream_read(floor.data_ptr(), floor.numel(), sink.data_ptr(), stream), "ts_bench_stream_read")

    out_m = torch.empty((4,), dtype=torch.float64, device=dev)
    variants = {"loss pair, unmasked (ts_photometric_loss_rgbd, two planes)": lambda: pair(rgb),
                "loss pair, masked (ts_photometric_loss_rgbd, two planes, TS_LOSS_MASKED)": masked_pair,
                "torch route: blend, unmasked pair, gradients times m": torch_route,
                f"streaming read of the masked pair's {moved} bytes": stream_read,
                "image_metrics, uint8 target": lambda: image_metrics(rgb, u8, out=out_m),
                "image_metrics, uint8 target, mask": lambda: image_metrics(rgb, u8, out=out_m, mask=mask)}
    for fn in variants.values():                               # warm-up, as bench.py warms its steps
        timed(fn, 10)
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, args.iters))
    rows = [{"call": k, "ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5), "ms_max": round(max(v), 5),
             "ms_rounds": [round(x, 5) for x in v]} for k, v in ms.items()]
    med = {k: statistics.median(v) for k, v in ms.items()}
    names = list(variants)
    result = {"height": h, "width": w, "iters": args.iters, "rounds": args.rounds, "mask_coverage": round(mask_coverage(mask), 4),
              "device": torch.cuda.get_device_name(dev), "rows": rows,
              "masked_over_unmasked": round(med[names[1]] / med[names[0]], 4),
              "masked_over_torch_route": round(med[names[1]] / med[names[2]], 4),
              "masked_over_streaming_floor": round(med[names[1]] / med[names[3]], 4),
              "masked_metrics_over_unmasked": round(med[names[5]] / med[names[4]], 4)}
    for note in args.note:
        key, _, value = note.partition("=")
        result[key] = value
    print(json.dumps(result, indent=1))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
