#!/usr/bin/env python
"""Times the undistortion kernel (tinysplat_amd.dataset.undistort_image) with device events after a
warm-up; prints one JSON line per measurement (ms per image, the median of ``--reps`` rounds of ten calls each, with the
minimum and maximum).

The image is ``--width`` x ``--height`` uniform random bytes seen through the ``opencv`` test camera scaled to that
size, resampled to the reference-mode matrix at the same size and, with ``--max-image-dimension``, to the centred matrix
at the smaller size (n x n sub-samples per pixel).  Per case:

  * ``kernel uint8`` / ``kernel float32``: one ts_undistort_image launch;
  * ``torch, grid kept``: what a caller writes without the kernel, the coordinate grid built once per camera and kept:
    the source to float [1,3,H,W], ``torch.nn.functional.grid_sample`` (bilinear, border padding, align_corners) per
    sub-sample grid, the mean, and the rounding back to uint8 [H',W',3];
  * ``torch, grid built``: the same with the grids built from the intrinsics in every call;
  * the kernel's bytes per second against the bytes it must move (the source read once, the target written once), as a
    share of the HBM peak, and the ratio of the compositions' times to the kernel's.  Each round times the kernel and then
    the compositions, so they alternate in one process;
  * the largest difference between the composition's and the kernel's bytes (grid_sample normalises coordinates to
    [-1, 1] and back in float32: one more rounding of the position).

    python tools/time_undistort.py [--width 4000] [--height 3000] [--max-image-dimension 1600] [--reps 20] [--out f.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd import dataset as D  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12               # bytes / s, the MI355X's HBM3E
INNER = 10                      # calls between one pair of events
OPENCV = ((85.0, 83.0, 46.3, 31.7), (-0.10, 0.02, 0.004, -0.003, 0.0, 0.0, 0.0, 0.0), (97, 61))   # tests/undistort_oracle.py


def scale_intrinsics(k, sx, sy):
    return np.array([k[0] * sx, k[1] * sy, (k[2] + 0.5) * sx - 0.5, (k[3] + 0.5) * sy - 0.5])


def supersample(w, h, ow, oh):
    return min(8, max(-(-w // ow), -(-h // oh)))


def grids(src_k, dst_k, d, size, out_size, dev):
    """the n x n normalised sampling grids [1,H',W',2] of grid_sample (align_corners=True) for one camera"""
    (w, h), (ow, oh) = size, out_size
    n = supersample(w, h, ow, oh)
    v, u = torch.meshgrid(torch.arange(oh, dtype=torch.float32, device=dev),
                          torch.arange(ow, dtype=torch.float32, device=dev), indexing="ij")
    out = []
    for b in range(n):
        for a in range(n):
            x = (u + ((a + 0.5) / n - 0.5) - dst_k[2]) / dst_k[0]
            y = (v + ((b + 0.5) / n - 0.5) - dst_k[3]) / dst_k[1]
            r2 = x * x + y * y
            rad = (1 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))) / (1 + r2 * (d[5] + r2 * (d[6] + r2 * d[7])))
            xd = x * rad + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
            yd = y * rad + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
            sx, sy = src_k[0] * xd + src_k[2], src_k[1] * yd + src_k[3]
            out.append(torch.stack([sx / (w - 1) * 2 - 1, sy / (h - 1) * 2 - 1], dim=-1)[None])
    return out


def composition(src_u8, gs):
    img = src_u8.permute(2, 0, 1)[None].to(torch.float32)
    acc = None
    for g in gs:
        s = F.grid_sample(img, g, mode="bilinear", padding_mode="border", align_corners=True)
        acc = s if acc is None else acc + s
    return torch.round(acc[0] / len(gs)).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--max-image-dimension", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device(DEV)
    w, h = args.width, args.height
    k, d, (w0, h0) = OPENCV
    d = np.asarray(d)
    src_k = scale_intrinsics(k, w / w0, h / h0)
    src = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(0))
    s = min(1.0, args.max_image_dimension / max(w, h))
    small = (max(1, int(w * s + 0.5)), max(1, int(h * s + 0.5)))
    kx, ky = small[0] / w, small[1] / h
    cen = D.centered_camera_matrix(src_k, d, w, h)
    cases = {"same size": (D.optimal_new_camera_matrix(src_k, d, w, h), (w, h)),
             f"downscaled to {small[0]}x{small[1]}": (np.array([cen[0] * kx, cen[1] * ky, (cen[2] + 0.5) * kx - 0.5,
                                                                (cen[3] + 0.5) * ky - 0.5]), small)}
    rows = []

    def emit(call, **kw):
        rows.append({"call": call, **kw, "width": w, "height": h, "reps": args.reps})
        print(json.dumps(rows[-1]), flush=True)

    for name, (dst_k, out_size) in cases.items():
        kept = grids(src_k, dst_k, d, (w, h), out_size, dev)
        calls = {"kernel uint8": lambda: D.undistort_image(src, src_k, dst_k, d, out_size),
                 "kernel float32": lambda: D.undistort_image(src, src_k, dst_k, d, out_size, dtype=torch.float32),
                 "torch, grid kept": lambda: composition(src, kept),
                 "torch, grid built": lambda: composition(src, grids(src_k, dst_k, d, (w, h), out_size, dev))}
        ms = {c: [] for c in calls}
        last = {}
        for rep in range(args.reps + 2):                                # two warm-up rounds: code objects, allocator
            for c, fn in calls.items():
                t, last[c] = event_ms(fn)
                if rep >= 2:
                    ms[c].append(t)
        shape = dict(case=name, out_width=out_size[0], out_height=out_size[1], samples_per_pixel=len(kept))
        for c, v in ms.items():
            emit(c, ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), **shape)
        kernel_ms = statistics.median(ms["kernel uint8"])
        moved = 3 * (w * h + out_size[0] * out_size[1])
        emit("kernel uint8 traffic", bytes=moved, gbytes_per_s=round(moved / kernel_ms / 1e6, 1),
             share_of_hbm_peak=round(moved / (kernel_ms * 1e-3) / HBM_PEAK, 4),
             grid_kept_over_kernel=round(statistics.median(ms["torch, grid kept"]) / kernel_ms, 2),
             grid_built_over_kernel=round(statistics.median(ms["torch, grid built"]) / kernel_ms, 2), **shape)
        diff = (last["torch, grid kept"].to(torch.int16) - last["kernel uint8"].to(torch.int16)).abs()
        emit("composition against the kernel", max_levels=int(diff.max()), share_differing=round(float((diff != 0).float().mean()), 6),
             **shape)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
