#!/usr/bin/env python
"""Times the .splat export (tinysplat_amd.formats) with device events after a warm-up; prints one
JSON line per measurement (ms per call, the median of ``--reps`` rounds of ten calls each, with the minimum and maximum).

  * the four stages of ``export_splat`` on N Gaussians: ``keys`` (ts_splat_keys), ``sort`` (the int64 composition and
    torch.sort), ``pack`` (ts_splat_pack with the order) and ``d2h`` (the record buffer to pageable host memory);
  * ``torch composition``: the same record buffer from torch ops with the same order - index_select, exp, sigmoid,
    stack, .to(uint8), cat: what one writes without the kernel.  Each round times the pack launch and then the
    composition, so the two alternate in one process; ``pack, model order`` is the launch without an order (no
    gather: the reads stream too);
  * the pack launch's achieved bytes per second against the bytes it must move: 56 B gathered + 8 B of index + 32 B
    written per record, as a share of the HBM peak;
  * ``unpack`` (ts_splat_unpack) and ``h2d`` of ``load_splat`` on the same records;
  * the share of bytes in which the composition differs from the kernel's records (its float32 quaternion norm and
    torch's own exp and sigmoid: a few bytes next to an integer).

    python tools/time_splat.py [--n 1000000] [--sh-degree 3] [--reps 20] [--out f.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd import _lib, formats  # noqa: E402
from tinysplat_amd.ops import _ptr, _stream  # noqa: E402
from tinysplat_amd.synthetic import make_scene  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12               # bytes / s, the MI355X's HBM3E
C0 = 0.28209479177387814
PACK_BYTES = 56 + 8 + 32        # per record: gathered, index, written


def composition(ts, order):
    """The record buffer from torch ops, given the order."""
    means, scales, dc, opac, quats = (t.index_select(0, order) for t in ts)
    n = means.shape[0]
    rgb = (255.0 * (0.5 + C0 * dc)).nan_to_num(nan=0.0).clamp(0.0, 255.0)
    alpha = (255.0 * torch.sigmoid(opac)).nan_to_num(nan=0.0).clamp(0.0, 255.0)
    norm = quats.norm(dim=1, keepdim=True)
    rot = torch.where((norm > 0) & torch.isfinite(norm), 128.0 * (quats / norm) + 128.0,
                      torch.tensor([256.0, 128.0, 128.0, 128.0], device=quats.device)).clamp(0.0, 255.0)
    return torch.cat([means.view(torch.uint8).view(n, 12), torch.exp(scales).view(torch.uint8).view(n, 12),
                      torch.cat([rgb, alpha, rot], 1).to(torch.uint8)], 1)


INNER = 10                      # calls between one pair of events: a single launch of tens of microseconds is near the
                                # events' own resolution


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
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device(DEV)
    model = make_scene(args.n, args.sh_degree, 1920, 1080, seed=0)[0].to(DEV)
    ts, _ = formats._splat_tensors(model)
    n = args.n
    lib = _lib.load()
    records = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    back = [torch.empty_like(t) for t in ts]

    def keys_stage():
        return formats._splat_keys(ts, dev)

    def pack_stage(order):
        assert lib.ts_splat_pack(n, n, *[_ptr(t) for t in ts], None if order is None else _ptr(order), _ptr(records),
                                 _stream(dev)) == 0
        return records

    def unpack_stage(src):
        assert lib.ts_splat_unpack(n, _ptr(src), *[_ptr(t) for t in back], _stream(dev)) == 0

    stages = {k: [] for k in ("keys", "sort", "pack, model order", "pack", "d2h", "torch composition", "h2d", "unpack")}
    for rep in range(args.reps + 2):                                    # two warm-up rounds: code objects, allocator
        ms_keys, keys = event_ms(keys_stage)
        ms_sort, order = event_ms(lambda: formats._order_from_keys(keys))
        ms_plain, _ = event_ms(lambda: pack_stage(None))
        ms_pack, _ = event_ms(lambda: pack_stage(order))
        ms_comp, composed = event_ms(lambda: composition(ts, order))
        ms_d2h, host = event_ms(lambda: records.cpu())
        ms_h2d, again = event_ms(lambda: host.to(dev))
        ms_unpack, _ = event_ms(lambda: unpack_stage(again))
        if rep >= 2:
            for k, v in zip(stages, (ms_keys, ms_sort, ms_plain, ms_pack, ms_d2h, ms_comp, ms_h2d, ms_unpack)):
                stages[k].append(v)
    rows = []
    shape = dict(n=n, sh_degree=args.sh_degree, reps=args.reps)

    def emit(call, **kw):
        rows.append({"call": call, **kw, **shape})
        print(json.dumps(rows[-1]), flush=True)

    for k, v in stages.items():
        emit(k, ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
    pack_ms = statistics.median(stages["pack"])
    emit("pack traffic", bytes_per_record=PACK_BYTES, bytes=PACK_BYTES * n,
         gbytes_per_s=round(PACK_BYTES * n / pack_ms / 1e6, 1),
         share_of_hbm_peak=round(PACK_BYTES * n / (pack_ms * 1e-3) / HBM_PEAK, 4),
         composition_over_pack=round(statistics.median(stages["torch composition"]) / pack_ms, 2))
    differ = composed != records
    emit("composition against the kernel", bytes_differing=int(differ.sum()),
         share=round(float(differ.float().mean()), 7), records_differing=int(differ.any(1).sum()))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
