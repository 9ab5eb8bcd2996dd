#!/usr/bin/env python
"""Times the label-vote walk with device events after a warm-up; one JSON line per row.

The scene is BASELINE config 3's geometry (1 M Gaussians at 1920 x 1080, seed 0; the colours play no part), the map a
150-class map of random 64 x 64 blocks.  Rows:

  * per view, each stage on its own: ``project_gaussians``, ``bin_gaussians`` (with its one host read), ``ts_pack_splats``
    and ``ts_label_votes`` with all 150 classes;
  * on the same lists and records, timed ALTERNATING with the vote launch in ``--rounds`` rounds of ``--iters`` calls:
    ``ts_raster_bwd`` + ``ts_reduce_partials`` at 4 channels with a one-hot image gradient - what four classes cost
    without the vote kernel, so ceil(C / 4) of them are the alternative;
  * the vote launch on a one-column map-less call (``gaussian_contributions``), on a single-label map, and on a map of
    24 x 24 blocks, which unlike the 64 x 64 ones are not aligned with the tiles: up to four columns per tile;
  * the vote launch on the same scene with ONE faint Gaussian in front that covers the whole image: every tile's wave
    adds to that Gaussian's row for every column it holds (atomics on a hot row).

    python tools/time_semantic.py [--n 1000000 --width 1920 --height 1080] [--iters 200] [--rounds 7] [--out FILE]
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd import _lib, ops  # noqa: E402
from tinysplat_amd.ops import _ptr, _stream  # noqa: E402
from tinysplat_amd.rasterizer import project_args  # noqa: E402
from tinysplat_amd.synthetic import SplatModel, make_scene  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def block_map(h, w, classes, block, seed):
    r = np.random.default_rng(seed)
    coarse = r.integers(0, classes, size=(-(-h // block), -(-w // block))).astype(np.uint8)
    return np.ascontiguousarray(np.kron(coarse, np.ones((block, block), np.uint8))[:h, :w])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device("cuda:0")
    n, w, h, C = args.n, args.width, args.height, args.classes
    model, cam = make_scene(n, 0, w, h, seed=0)
    model = model.to(dev)
    lib, s = _lib.load(), _stream(dev)
    labels_np = block_map(h, w, C, args.block, 1)
    labels = torch.from_numpy(labels_np).to(dev)
    one_label = torch.zeros_like(labels)
    class_map = torch.full((256,), 255, dtype=torch.uint8)
    class_map[:C] = torch.arange(C, dtype=torch.uint8)
    class_map = class_map.to(dev)

    with torch.no_grad():
        pa = project_args(model, cam, (w, h), dev)
        xys, depths, radii, conics, nth, _ = ops.project_gaussians(*pa)
        b = ops.bin_gaussians(xys, depths, radii, nth, h, w, use_cache=False)
        total = b.num_intersects
        colors = torch.zeros((n, 4), device=dev)
        splats = torch.empty((n, 12), device=dev)
        votes = torch.zeros((n, C), dtype=torch.int64, device=dev)
        votes1 = torch.zeros((n, 1), dtype=torch.int64, device=dev)

        def project():
            ops.project_gaussians(*pa)

        def bins():
            ops.bin_gaussians(xys, depths, radii, nth, h, w, use_cache=False)

        def pack():
            _lib.check(lib.ts_pack_splats(n, 4, _lib.RASTER_LOGIT_OPACITY, _ptr(xys), _ptr(radii), _ptr(conics), _ptr(colors),
                                          _ptr(model.opacities), _ptr(b.cum_tiles_hit), b.cam, None, _ptr(splats), s),
                       "ts_pack_splats")

        def vote():
            _lib.check(lib.ts_label_votes(0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted), _ptr(splats),
                                          _ptr(labels), _ptr(class_map), C, _ptr(votes), s), "ts_label_votes")

        def vote_one_label():
            _lib.check(lib.ts_label_votes(0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted), _ptr(splats),
                                          _ptr(one_label), _ptr(class_map), C, _ptr(votes), s), "ts_label_votes")

        # 64 x 64 blocks are aligned with the 16 x 16 tiles (one column per tile); 24 x 24 blocks give a tile up to four
        labels_24 = torch.from_numpy(block_map(h, w, C, 24, 2)).to(dev)

        def vote_24():
            _lib.check(lib.ts_label_votes(0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted), _ptr(splats),
                                          _ptr(labels_24), _ptr(class_map), C, _ptr(votes), s), "ts_label_votes")

        def vote_no_map():
            _lib.check(lib.ts_label_votes(0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted), _ptr(splats),
                                          None, None, 1, _ptr(votes1), s), "ts_label_votes")

        # the alternative: the backward compositing launch with a one-hot image gradient, four classes per pass
        pack()
        background = torch.zeros(4, device=dev)
        out_img = torch.empty((h, w, 4), device=dev)
        final_T = torch.empty((h, w), device=dev)
        final_idx = torch.empty((h, w), dtype=torch.int32, device=dev)
        _lib.check(lib.ts_raster_fwd(4, 0, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted), _ptr(splats),
                                     _ptr(background), _ptr(out_img), _ptr(final_T), _ptr(final_idx), None, s), "ts_raster_fwd")
        v_out = torch.stack([(labels == c) for c in range(4)], dim=-1).to(torch.float32).contiguous()
        partials = torch.empty((max(total, 1), _lib.PARTIAL_ROW_FLOATS), device=dev)
        row_flags = torch.empty((max(total, 1),), dtype=torch.uint8, device=dev)
        flat = torch.empty((n * 10,), device=dev)
        v_xy, v_conic, v_colors, v_opacity = flat[:2 * n], flat[2 * n:5 * n], flat[5 * n:9 * n], flat[9 * n:]

        def bwd_pair():
            _lib.check(lib.ts_raster_bwd(4, 0, total, b.cam, _ptr(b.tile_bins), _ptr(b.gaussian_ids_sorted), _ptr(splats),
                                         _ptr(background), _ptr(final_T), _ptr(final_idx), _ptr(v_out), None, None,
                                         _ptr(partials), _ptr(row_flags), s), "ts_raster_bwd")
            _lib.check(lib.ts_reduce_partials(n, 4, 1, _ptr(b.num_tiles_hit), _ptr(b.cum_tiles_hit), _ptr(partials),
                                              _ptr(row_flags), _ptr(splats), _ptr(v_xy), _ptr(v_conic), _ptr(v_colors),
                                              _ptr(v_opacity), None, None, s), "ts_reduce_partials")

        sides = {"project_gaussians": project, "bin_gaussians (one host read inside)": bins, "ts_pack_splats": pack,
                 f"ts_label_votes, {C} classes, {args.block} x {args.block} blocks": vote,
                 "ts_raster_bwd + ts_reduce_partials, 4 channels, one-hot gradient (4 classes)": bwd_pair,
                 "ts_label_votes, one label everywhere": vote_one_label,
                 "ts_label_votes, no map, 1 column (gaussian_contributions)": vote_no_map,
                 f"ts_label_votes, {C} classes, 24 x 24 blocks (up to four columns per tile)": vote_24}
        for fn in sides.values():
            timed(fn, max(3, args.iters // 4))
        ms = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                ms[k].append(timed(fn, args.iters))
        # a hot row: the same scene behind one faint Gaussian (alpha 0.05) that covers every pixel
        front = [torch.tensor([[0.0, 0.0, 1.0]]), torch.zeros(1, 3), torch.zeros(1, 0, 3), torch.full((1, 3), math.log(50.0)),
                 torch.tensor([[1.0, 0.0, 0.0, 0.0]]), torch.tensor([[math.log(0.05 / 0.95)]])]
        hot = SplatModel(*[torch.cat([p, f.to(dev)]) for p, f in zip(model.parameters(), front)], active_sh_degree=0,
                         background=model.background)
        hx, hd, hr, hc, hn, _ = ops.project_gaussians(*project_args(hot, cam, (w, h), dev))
        hb = ops.bin_gaussians(hx, hd, hr, hn, h, w, use_cache=False)
        hsplats = torch.empty((n + 1, 12), device=dev)
        hvotes = torch.zeros((n + 1, C), dtype=torch.int64, device=dev)
        _lib.check(lib.ts_pack_splats(n + 1, 4, _lib.RASTER_LOGIT_OPACITY, _ptr(hx), _ptr(hr), _ptr(hc),
                                      _ptr(torch.zeros((n + 1, 4), device=dev)), _ptr(hot.opacities), _ptr(hb.cum_tiles_hit),
                                      hb.cam, None, _ptr(hsplats), s), "ts_pack_splats")

        def vote_hot():
            _lib.check(lib.ts_label_votes(0, hb.cam, _ptr(hb.tile_bins), _ptr(hb.gaussian_ids_sorted), _ptr(hsplats),
                                          _ptr(labels), _ptr(class_map), C, _ptr(hvotes), s), "ts_label_votes")

        timed(vote_hot, max(3, args.iters // 4))
        hot_ms = [timed(vote_hot, args.iters) for _ in range(args.rounds)]
        torch.cuda.synchronize()
        hot_row_votes = int((hvotes[n] > 0).sum())
    rows = []
    for k, v in ms.items():
        rows.append({"call": k, "gaussians": n, "width": w, "height": h, "intersections": int(total), "iters": args.iters,
                     "rounds": args.rounds, "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                     "ms_max": round(max(v), 4)})
    vote_ms, pair_ms = rows[3]["ms_median"], rows[4]["ms_median"]
    passes = -(-C // 4)
    rows.append({"call": "one vote launch / one backward pair", "ratio": round(vote_ms / pair_ms, 4),
                 "all_classes_by_votes_ms": vote_ms, "all_classes_by_backward_ms": round(passes * pair_ms, 3),
                 "backward_passes": passes})
    rows.append({"call": f"ts_label_votes, {C} classes, one more Gaussian in front covering every tile",
                 "intersections": int(hb.num_intersects), "columns_of_the_hot_row_with_votes": hot_row_votes,
                 "ms_median": round(statistics.median(hot_ms), 4), "ms_min": round(min(hot_ms), 4),
                 "ms_max": round(max(hot_ms), 4)})
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
