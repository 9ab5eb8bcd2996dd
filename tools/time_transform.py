#!/usr/bin/env python
"""Times the scene transform: one ``ts_transform_gaussians`` launch on a model of 1M Gaussians at SH
degrees 0 and 3 (and ``edit.transform_gaussians``, which also builds the host arrays and allocates the outputs), against
(a) a device-to-device copy of the same bytes and (b) the torch equivalent (``@``, a quaternion product and one ``einsum``
per band), all with device events, interleaved in blocks.

    python tools/time_transform.py --json profiles/transform_times.json

Prints one JSON object.  Needs a GPU."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--degrees", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per variant, interleaved")
    ap.add_argument("--repeats", type=int, default=20, help="launches per block")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def torch_equivalent(model, t, mats):
    """The same result in plain torch, for the comparison only (its sums are in another order)."""
    import torch
    dev = model.means.device
    m = torch.as_tensor(t.scale * t.rotation, dtype=torch.float32, device=dev)
    tr = torch.as_tensor(t.translation.copy(), dtype=torch.float32, device=dev)
    r = torch.as_tensor(t.quat(), dtype=torch.float32, device=dev)
    mats = [torch.as_tensor(d, dtype=torch.float32, device=dev) for d in mats]
    log_s = math.log(t.scale)

    def run():
        means = model.means @ m.T + tr
        scales = model.scales + log_s
        w, x, y, z = model.quats.unbind(-1)
        quats = torch.stack([r[0] * w - r[1] * x - r[2] * y - r[3] * z, r[0] * x + r[1] * w + r[2] * z - r[3] * y,
                             r[0] * y - r[1] * z + r[2] * w + r[3] * x, r[0] * z + r[1] * y - r[2] * x + r[3] * w], -1)
        bands = [torch.einsum("jk,nkc->njc", d, model.colors_rest[:, l * l - 1:(l + 1) ** 2 - 1])
                 for l, d in enumerate(mats, start=1)]
        rest = torch.cat(bands, 1) if bands else model.colors_rest.clone()
        return means, scales, quats, rest
    return run


def time_degree(args, degree):
    import torch
    from tinysplat_amd import edit
    from tinysplat_amd.synthetic import make_scene
    dev = "cuda:0"
    model = make_scene(args.gaussians, degree, 64, 48, seed=0)[0].to(dev)
    t = edit.Sim3.from_quat((0.3, -0.5, 0.7, 0.2), (0.5, -1.0, 2.0), 2.5)
    tensors = [model.means, model.scales, model.quats, model.colors_rest]
    copies = [torch.empty_like(p) for p in tensors]
    nbytes = 2 * sum(p.numel() * 4 for p in tensors)                   # read once, written once

    def copy():
        for dst, src in zip(copies, tensors):
            dst.copy_(src)
    # the launch alone: host arrays and outputs made once (transform_gaussians builds them on every call)
    from tinysplat_amd import _lib
    from tinysplat_amd.ops import _ptr, _stream
    lib = _lib.load()
    (xform, xform_p), (quat, quat_p), log_scale, (sh, sh_p) = (
        edit._float_array(a) if hasattr(a, "shape") else a for a in edit.kernel_arguments(t, degree))
    n, k_rest = model.means.shape[0], model.colors_rest.shape[1]
    pointers = [_ptr(p) if p.numel() else None for p in tensors + copies]

    def launch():
        _lib.check(lib.ts_transform_gaussians(n, k_rest, xform_p, quat_p, log_scale, sh_p if sh.size else None, None,
                                              *pointers, _stream(torch.device(dev))), "ts_transform_gaussians")
    variants = {"ts_transform_gaussians": launch, "transform_gaussians": lambda: edit.transform_gaussians(model, t),
                "copy": copy, "torch": torch_equivalent(model, t, edit.sh_rotation_matrices(t.rotation, degree))}
    got, want = edit.transform_gaussians(model, t), variants["torch"]()
    worst = max(float((a - b).abs().max()) for a, b in zip((got.means, got.scales, got.quats, got.colors_rest), want)
                if a.numel())
    for fn in variants.values():                                       # warm-up
        for _ in range(3):
            fn()
    samples = {name: [] for name in variants}
    for _block in range(args.blocks):                                  # interleaved blocks: drift hits every variant alike
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.repeats):
                fn()
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / args.repeats * 1e3)
    out = {"degree": degree, "bytes": nbytes, "max_abs_difference_from_torch": worst}
    for name, v in samples.items():
        med = statistics.median(v)
        out[name] = {"us_median": med, "us_min": min(v), "us_max": max(v), "tb_per_s": nbytes / med / 1e6}
    out["fraction_of_copy_rate"] = out["copy"]["us_median"] / out["ts_transform_gaussians"]["us_median"]
    return out


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    result = {"gaussians": args.gaussians, "blocks": args.blocks, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "runs": [time_degree(args, d) for d in args.degrees]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
