#!/usr/bin/env python
"""Times the evaluation metrics with device events after a warm-up; one JSON line per row.

  * the entry: ``ts_image_metrics`` with a uint8 target against the training loss's forward (``ts_photometric_loss_rgbd``
    without a gradient image + ``ts_photometric_loss_reduce``) on the float target, both on preallocated workspaces,
    timed ALTERNATING in ``--rounds`` rounds of ``--iters`` calls each; per side the median and the smallest and largest
    round (the run-to-run spread of this very call), the bytes the algorithm moves computed from the shapes, and their
    share of the HBM rate at the median;
  * ``evaluate`` per view on BASELINE config 3 (1 M Gaussians, SH 3, 1920 x 1080) with and without the metrics launches:
    what an evaluation adds to a ``render_view``.

    python tools/time_metrics.py [--width 1920 --height 1080] [--iters 2000] [--rounds 7] [--n 1000000] [--out FILE]
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd import _lib, evaluate  # noqa: E402
from tinysplat_amd import metrics as M  # noqa: E402
from tinysplat_amd.ops import _ptr, _stream  # noqa: E402
from tinysplat_amd.synthetic import make_scene  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12        # bytes / s: the data sheet's rate, and what a float4 copy reaches


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def entry_rows(h, w, iters, rounds, dev):
    g = torch.Generator().manual_seed(h * w)
    img = torch.rand(h, w, 3, generator=g)
    tgt = (img + 0.2 * torch.randn(h, w, 3, generator=g)).clamp(0, 1)
    u8 = (tgt * 255.0).round().to(torch.uint8).to(dev)
    img, tgt = img.to(dev), tgt.to(dev)
    lib = _lib.load()
    ws_m = torch.empty((int(lib.ts_image_metrics_ws_bytes(h, w)),), dtype=torch.uint8, device=dev)
    out_m = torch.empty((4,), dtype=torch.float64, device=dev)
    ws_l = torch.empty((int(lib.ts_photometric_ws_floats(h, w)),), dtype=torch.float32, device=dev)
    out_l = torch.empty((4,), dtype=torch.float32, device=dev)
    stream = _stream(dev)
    w_l1, w_ssim = 0.8 / (3.0 * h * w), -0.2 / (3.0 * (h - 10) * (w - 10))

    def metrics():
        _lib.check(lib.ts_image_metrics(h, w, 3, _ptr(img), _ptr(u8), 1, _ptr(ws_m), _ptr(out_m), stream), "ts_image_metrics")

    loss = _lib.TsLoss(height=h, width=w, pixel_floats=3, image=_ptr(img), target=_ptr(tgt), w_l1=w_l1, w_ssim=w_ssim,
                       ws=_ptr(ws_l))

    def loss_forward():
        _lib.check(lib.ts_photometric_loss_rgbd(ctypes.byref(loss), stream), "ts_photometric_loss_rgbd")
        _lib.check(lib.ts_photometric_loss_reduce(h, w, w_l1, w_ssim, 0.0, _ptr(ws_l), _ptr(out_l), stream),
                   "ts_photometric_loss_reduce")

    sides = {"ts_image_metrics, uint8 target": metrics,
             "ts_photometric_loss_rgbd forward + reduce, float target, no gradient": loss_forward}
    for fn in sides.values():
        timed(fn, max(50, iters // 10))
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, iters))
    px, mp = h * w, (h - 10) * (w - 10)
    moved = {"ts_image_metrics, uint8 target": 12 * px + 3 * px,                       # image + bytes, read once
             "ts_photometric_loss_rgbd forward + reduce, float target, no gradient": 12 * px + 12 * px + 36 * mp}   # + 9 maps written
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        rows.append({"call": k, "height": h, "width": w, "iters": iters, "rounds": rounds, "ms_median": round(med, 5),
                     "ms_min": round(min(v), 5), "ms_max": round(max(v), 5), "bytes": moved[k],
                     "hbm_share_of_8.0TBps": round(moved[k] / (med * 1e-3) / HBM_SPEC, 4),
                     "hbm_share_of_6.29TBps": round(moved[k] / (med * 1e-3) / HBM_COPY, 4)})
    a, b = rows
    spread = max(a["ms_max"] - a["ms_min"], b["ms_max"] - b["ms_min"])
    rows.append({"call": "metrics - loss forward", "ms_median_difference": round(a["ms_median"] - b["ms_median"], 5),
                 "ms_spread_of_this_call": round(spread, 5),
                 "metrics_not_slower_beyond_spread": bool(a["ms_median"] - b["ms_median"] <= spread)})
    return rows


def evaluate_rows(n, h, w, views, reps, dev):
    model, cam = make_scene(n, 3, w, h)
    model = model.to(dev)
    cams = [cam] * views
    with torch.no_grad():
        from tinysplat_amd import GaussianRasterizer
        own = GaussianRasterizer(model, cams, device=dev)(cam, None, 3)[0]
        targets = [(own * 255.0).round().to(torch.uint8)] * views

    def per_view():
        evaluate(model, cams, targets, dev)                  # warm-up
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            evaluate(model, cams, targets, dev)              # ends in its device-to-host copy
            t.append((time.perf_counter() - t0) * 1e3 / views)
        return t
    with_metrics = per_view()
    keep = M.image_metrics
    M.image_metrics = lambda image, target, out=None: out    # the same loop without the two launches (the table stays unset)
    try:
        without = per_view()
    finally:
        M.image_metrics = keep
    return [{"call": "evaluate per view", "gaussians": n, "height": h, "width": w, "views": views, "reps": reps,
             "ms_median": round(statistics.median(with_metrics), 4), "ms_min": round(min(with_metrics), 4),
             "ms_max": round(max(with_metrics), 4)},
            {"call": "evaluate per view, metrics launches removed", "gaussians": n, "height": h, "width": w,
             "views": views, "reps": reps, "ms_median": round(statistics.median(without), 4),
             "ms_min": round(min(without), 4), "ms_max": round(max(without), 4)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, default=1_000_000, help="Gaussians of the evaluate timing; 0 skips it")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device("cuda:0")
    rows = entry_rows(args.height, args.width, args.iters, args.rounds, dev)
    if args.n > 0:
        rows += evaluate_rows(args.n, args.height, args.width, args.views, args.reps, dev)
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
