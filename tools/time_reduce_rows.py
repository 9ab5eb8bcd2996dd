#!/usr/bin/env python
"""Times the gradient-row reduction (``ts_reduce_partials``) on synthetic inputs of the size of
BASELINE configs[2]: 1M Gaussians whose slot counts are the tile counts of boxes of (1 + Poisson(1.5))^2 tiles - mean 6.25,
as in that frame - and 12-float rows of which none, 39 % (the frame's share) and all are flagged with the current
generation; the other flag bytes hold an older generation, as a persistent flag array leaves them.  "none" fetches no row
at all: it is the launch's cost that does not depend on the rows.  Device events around ``--repeats`` launches, the three
cases interleaved in blocks after untimed warm-up launches.

    python tools/time_reduce_rows.py --json profiles/reduce_rows_times.json

``TS_LIB_PATH`` / ``TS_ALLOW_VARIANT_LIB=1`` time another build of the library (``-DTS_REDUCE_ROWS=2``: two flagged rows
per step; ``-DTS_REDUCE_BLOCK=128``); the result records the library's flags.  Prints one JSON object.  Needs a GPU."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GEN = 7                     # the pass's generation; stale bytes carry GEN - 1
CASES = (("none", 0.0), ("frame", 0.39), ("all", 1.0))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--channels", type=int, default=3, choices=(3, 4))
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per case, interleaved")
    ap.add_argument("--repeats", type=int, default=20, help="launches per block")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def make_inputs(n, dev):
    """Counts, their running sum, rows, records and one flag array per case."""
    import torch
    g = torch.Generator().manual_seed(0)
    lam = torch.full((n,), 1.5)
    cnt = ((1 + torch.poisson(lam, generator=g)) * (1 + torch.poisson(lam, generator=g))).to(torch.int32)
    cum = torch.cumsum(cnt, 0, dtype=torch.int64)
    total = int(cum[-1])
    assert total < 2 ** 31
    partials = torch.randn(total, 12, generator=g)
    splats = torch.rand(n, 12, generator=g) * 0.9 + 0.05
    flags = {}
    for name, share in CASES:
        f = torch.full((total,), GEN - 1, dtype=torch.uint8)
        f[torch.rand(total, generator=g) < share] = GEN
        flags[name] = f.to(dev)
    return cnt.to(dev), cum.to(torch.int32).to(dev), partials.to(dev), splats.to(dev), flags, total


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd import _lib
    from tinysplat_amd.ops import _ptr, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n, ch = args.gaussians, args.channels
    cnt, cum, partials, splats, flags, total = make_inputs(n, dev)
    v_xy, v_conic = torch.empty(n, 2, device=dev), torch.empty(n, 3, device=dev)
    v_colors, v_opacity = torch.empty(n, ch, device=dev), torch.empty(n, device=dev)
    stream = _stream(dev)

    def launch(f):
        def run():
            _lib.check(lib.ts_reduce_partials(n, ch, 1 | (GEN << 8), _ptr(cnt), _ptr(cum), _ptr(partials), _ptr(f),
                                              _ptr(splats), _ptr(v_xy), _ptr(v_conic), _ptr(v_colors), _ptr(v_opacity),
                                              None, None, stream), "ts_reduce_partials")
        return run
    variants = {name: launch(flags[name]) for name, _ in CASES}
    for fn in variants.values():                                       # warm-up, untimed
        for _ in range(3):
            fn()
    samples = {name: [] for name in variants}
    for _block in range(args.blocks):                                  # interleaved blocks: drift hits every case alike
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.repeats):
                fn()
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / args.repeats * 1e3)
    stamp = _lib.LIB_PATH.with_suffix(_lib.LIB_PATH.suffix + ".flags")
    lib_flags = sorted({f for f in stamp.read_text().split() if f.startswith("-DTS_")}) if stamp.exists() else []
    result = {"gaussians": n, "channels": ch, "slots": total, "mean_slots": total / n, "max_slots": int(cnt.max()),
              "blocks": args.blocks, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "library": str(_lib.LIB_PATH), "library_flags": lib_flags, "cases": {}}
    for name, share in CASES:
        v = samples[name]
        rows = int((flags[name] == GEN).sum())
        result["cases"][name] = {"flagged_share": share, "flagged_rows": rows, "us_median": statistics.median(v),
                                 "us_min": min(v), "us_max": max(v)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
