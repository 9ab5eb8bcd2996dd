#!/usr/bin/env python
"""Times one viewer request on config 3 (1 M Gaussians, SH degree 3) at 1920 x 1080, as a client sees it: from the pose to
the JPEG file in host memory.  Prints one JSON line per measurement (ms: the median of ``--reps`` requests timed on the
host clock around a synchronising call, with the spread between the fastest and the slowest).

  * ``render + host encode``: what the package offered before - ``ViewRenderer.render(as_uint8=True)``, 6.2 MB across
    PCIe, then Pillow's (libjpeg's) ``save(format="JPEG", quality=90)`` on the host;
  * its two parts, each on its own;
  * ``render_jpeg``: the frame encoded on the GPU, only the file crosses;
  * ``part ...``: the encoder's launches on their own (``ops.kernel_timer``: device events around the C entry) and the
    render they follow;
  * the bytes that crossed PCIe for each.

    python tools/time_jpeg.py [--n 1000000] [--reps 30] [--quality 90] [--subsampling 420] [--out time_jpeg.jsonl]
"""
import argparse
import io
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd.ops import kernel_timer  # noqa: E402
from tinysplat_amd.synthetic import make_scene  # noqa: E402
from tinysplat_amd.viewer import ViewRenderer  # noqa: E402

DEV = "cuda:0"
PIL_SUB = {"444": 0, "420": 2}


def host_timed(fn, reps, warm=3):
    """Wall-clock ms of ``fn`` (which leaves nothing running on the device) -> median, fastest, slowest."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", choices=("420", "444"), default="420")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    from PIL import Image
    rows = []

    def emit(call, ms, lo=None, hi=None, **kw):
        row = {"call": call, "ms": round(ms, 4)}
        if lo is not None:
            row.update(fastest_ms=round(lo, 4), slowest_ms=round(hi, 4), spread_ms=round(hi - lo, 4))
        rows.append({**row, **kw})
        print(json.dumps(rows[-1]), flush=True)

    w, h = args.width, args.height
    model, cam = make_scene(args.n, 3, w, h, seed=0)
    vr = ViewRenderer(model.to(DEV), cam, DEV)
    pose = ([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
    shape = dict(n=args.n, width=w, height=h, quality=args.quality, subsampling=args.subsampling, reps=args.reps)

    def host_encode(u8):
        buf = io.BytesIO()
        Image.fromarray(u8).save(buf, format="JPEG", quality=args.quality, subsampling=PIL_SUB[args.subsampling])
        return buf.getvalue()

    def parent():
        return host_encode(vr.render(*pose, as_uint8=True))

    def ours():
        return vr.render_jpeg(*pose, args.quality, args.subsampling)
    theirs, mine = parent(), ours()
    u8 = vr.render(*pose, as_uint8=True).copy()
    p_ms = host_timed(parent, args.reps)
    emit("render + host encode", *p_ms, pcie_bytes=int(u8.nbytes), file_bytes=len(theirs), **shape)
    emit("part render(as_uint8=True)", *host_timed(lambda: vr.render(*pose, as_uint8=True), args.reps), **shape)
    emit("part host encode (libjpeg)", *host_timed(lambda: host_encode(u8), args.reps), **shape)
    o_ms = host_timed(ours, args.reps)
    emit("render_jpeg", *o_ms, pcie_bytes=len(mine) + 4, file_bytes=len(mine), **shape)
    emit("saved per request", p_ms[0] - o_ms[0], spread_of_both_ms=round((p_ms[2] - p_ms[1]) + (o_ms[2] - o_ms[1]), 4),
         wins=bool(p_ms[0] - o_ms[0] > (p_ms[2] - p_ms[1]) + (o_ms[2] - o_ms[1])), **shape)

    # the device time of the parts: events around the render's entries and the encoder's entry
    frame = vr._frame(*pose)
    enc = next(iter(vr._encoders.values()))
    for _ in range(3):
        enc.encode(frame, args.quality)
    kernel_timer.start()
    for _ in range(args.reps):
        enc.launch(frame, args.quality)
    torch.cuda.synchronize()
    parts = kernel_timer.stop()
    enc.collect()
    for name, (launches, mean_ms) in sorted(parts.items()):
        emit("part " + name + " (device, per frame)", mean_ms, launches=launches, **shape)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.reps):
        vr._frame(*pose)
    b.record()
    torch.cuda.synchronize()
    render_ms = a.elapsed_time(b) / args.reps
    emit("part render (device, per frame)", render_ms, **shape)
    if "ts_jpeg_encode" in parts:
        emit("encoder kernels over render", parts["ts_jpeg_encode"][1] / render_ms, **shape)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
