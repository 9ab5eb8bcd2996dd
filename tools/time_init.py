#!/usr/bin/env python
"""Times knn_points (k = 4 and k = 16, self-search) and from_pcd at 1 M points for each cloud of
tests/test_gpu_init.py, with device events after a warm-up; prints one JSON line per (cloud, call) with ms per
call and the number of queries that took the brute-force fallback.  The cloud of identical points is timed at
20 k points only: one grid cell holds every point, so its search is quadratic (1e12 distances at 1 M).

    python tools/time_init.py [--n 1000000] [--reps 10] [--out time_init.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from test_gpu_init import KINDS, cloud  # noqa: E402
from tinysplat_amd import PointCloud, from_pcd, knn_points  # noqa: E402


def timed(fn, reps):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    rows = []
    for kind in KINDS:
        n = min(args.n, 20_000) if kind == "identical" else args.n
        pts = cloud(kind, n=n)
        p = pts.to("cuda:0")
        for k in (4, 16):
            ms = timed(lambda: knn_points(p, p, k), args.reps)
            st = knn_points(p, p, k, return_stats=True)[2].tolist()
            rows.append({"cloud": kind, "n": n, "call": f"knn_points k={k}", "ms": round(ms, 3),
                         "fallback_queries": st[0], "max_rings": st[1]})
            print(json.dumps(rows[-1]), flush=True)
        colors = torch.randint(0, 256, (n, 3), dtype=torch.uint8)
        pcd = PointCloud(torch.arange(n), pts, colors, torch.zeros(n))
        ms = timed(lambda: from_pcd(pcd, sh_degree=3, generator=torch.Generator().manual_seed(0)), args.reps)
        rows.append({"cloud": kind, "n": n, "call": "from_pcd (host rand + uploads included)", "ms": round(ms, 3)})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
