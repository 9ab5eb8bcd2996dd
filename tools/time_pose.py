#!/usr/bin/env python
"""Times the pose gradient: ``ts_pose_grad`` (two launches) on 1M rows - with dense random gradient
rows and with the rows a backward pass through the BASELINE configs[2] frame (1M Gaussians, SH 3, 1920x1080) leaves, most
of them zero - against (a) a device-to-device copy of the same 56 bytes per row, (b) ``ts_bench_stream_read`` over as many
bytes and (c) the torch expression (``cross``, ``einsum``, ``sum`` in double), all with device events, interleaved in
blocks after untimed warm-up launches.  Then ``TrainStep`` on that frame four ways - the fused Adam step, the two-launch
step, and the two-launch step with ``poses`` over eight views in turn and over one view - whose differences are the
unfused Adam and the pose update (reduction, the 48-byte copy to the host and the host's Adam and retraction; with one
view also the wait for the step before).

    python tools/time_pose.py --json profiles/pose_times.json

``TS_LIB_PATH`` / ``TS_ALLOW_VARIANT_LIB=1`` time another build of the library (``-DTS_POSE_LDS_BUTTERFLY=1``: the wave's
sum through LDS); the result records the library's flags.  Prints one JSON object.  Needs a GPU."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per variant, interleaved")
    ap.add_argument("--repeats", type=int, default=20, help="launches per block")
    ap.add_argument("--steps", type=int, default=30, help="timed steps of each TrainStep run, in blocks of 10; 0 skips them")
    ap.add_argument("--json", type=str, default=None, help="also write the result to this file")
    return ap.parse_args(argv)


def torch_equivalent(view, means, quats, v_means, v_quats):
    """The six sums in plain torch double, for the comparison only (its sums are in another order)."""
    import torch
    V = torch.as_tensor(view, dtype=torch.float64, device=means.device)
    R, t = V[:3, :3], V[:3, 3]

    def run():
        m, q, g, h = means.double(), quats.double(), v_means.double(), v_quats.double()
        p = m @ R.T + t
        gc = g @ R.T
        w, x, y, z = q.unbind(-1)
        e = torch.stack([torch.stack([-x, w, -z, y], -1), torch.stack([-y, z, w, -x], -1), torch.stack([-z, -y, x, w], -1)], 1)
        tau = 0.5 * torch.einsum("nk,njk->nj", h, e)
        return torch.cat([gc.sum(0), (torch.linalg.cross(p, gc) + tau @ R.T).sum(0)])
    return run


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


def frame_gradients(args, dev):
    """(model, camera) of the configs[2] frame with the gradient rows of one backward pass on means and quats."""
    import torch
    from tinysplat_amd import GaussianRasterizer
    from tinysplat_amd.synthetic import make_scene
    from tinysplat_amd.training import planes_loss
    model, cam = make_scene(args.gaussians, 3, args.width, args.height, seed=0)
    model = model.to(dev).requires_grad_(True)
    target = torch.rand(args.height, args.width, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    rgb, extras = GaussianRasterizer(model, None, device=torch.device(dev))(cam, None, 3)
    planes_loss(rgb.contiguous(), extras["depth"].contiguous(), target)[0].backward()
    return model, cam


def time_kernel(args):
    import torch
    from tinysplat_amd import _lib, pose
    from tinysplat_amd.ops import _ptr, _stream
    dev = "cuda:0"
    lib = _lib.load()
    model, cam = frame_gradients(args, dev)
    n = int(model.means.shape[0])
    gen = torch.Generator().manual_seed(3)
    rows = {"frame": (model.means.grad, model.quats.grad),
            "dense": (torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, 4, generator=gen).to(dev))}
    means, quats = model.means.detach(), model.quats.detach()
    view = pose._view34(cam)
    view_p = view.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ws = torch.empty((int(lib.ts_pose_ws_bytes(n)) // 8,), dtype=torch.float64, device=dev)
    out6 = torch.empty((6,), dtype=torch.float64, device=dev)
    nbytes = 56 * n
    flat = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev).normal_()
    sink = torch.zeros((1,), dtype=torch.float32, device=dev)
    runs = []
    for name, (v_means, v_quats) in rows.items():
        tensors = [means, quats, v_means, v_quats]
        copies = [torch.empty_like(t) for t in tensors]

        def copy():
            for dst, src in zip(copies, tensors):
                dst.copy_(src)

        def launch():
            _lib.check(lib.ts_pose_grad(n, view_p, _ptr(means), _ptr(quats), _ptr(v_means), _ptr(v_quats), _ptr(ws),
                                        _ptr(out6), _stream(torch.device(dev))), "ts_pose_grad")

        def stream_read():
            _lib.check(lib.ts_bench_stream_read(_ptr(flat), flat.numel(), _ptr(sink), _stream(torch.device(dev))),
                       "ts_bench_stream_read")
        variants = {"ts_pose_grad": launch, "pose_gradient": lambda: pose.pose_gradient(model, cam, v_means, v_quats),
                    "copy": copy, "stream_read": stream_read, "torch": torch_equivalent(view, *tensors)}
        got, want = pose.pose_gradient(model, cam, v_means, v_quats), variants["torch"]()
        samples = timed(variants, args.blocks, args.repeats)
        zero = float(((v_means == 0).all(1) & (v_quats == 0).all(1)).float().mean())
        out = {"rows": name, "bytes_read": nbytes, "zero_gradient_rows": zero, "launches": 2,
               "max_relative_difference_from_torch": float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))}
        for key, v in samples.items():
            med = statistics.median(v)
            out[key] = {"us_median": med, "us_min": min(v), "us_max": max(v)}
        out["ts_pose_grad"]["tb_per_s"] = nbytes / out["ts_pose_grad"]["us_median"] / 1e6
        out["stream_read"]["tb_per_s"] = nbytes / out["stream_read"]["us_median"] / 1e6
        out["copy"]["tb_per_s_read_plus_written"] = 2 * nbytes / out["copy"]["us_median"] / 1e6
        out["fraction_of_stream_read_rate"] = out["stream_read"]["us_median"] / out["ts_pose_grad"]["us_median"]
        runs.append(out)
    return runs


def time_train_step(args):
    import torch
    from tinysplat_amd.pose import PoseConfig, PoseModel
    from tinysplat_amd.synthetic import make_scene
    from tinysplat_amd.training import TrainStep
    h, w, dev = args.height, args.width, "cuda:0"
    target = torch.rand(h, w, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    runs = {}
    # "poses": eight views of the one camera in turn, as a training run cycles through its cameras - a view's update is
    # applied when the view comes up again; "poses_one_view": the same view every step, so every step waits for the last
    views = {"poses": 8, "poses_one_view": 1}
    for name in ("fused", "two_launch", "poses", "poses_one_view"):
        model, cam = make_scene(args.gaussians, 3, w, h, seed=0)
        model = model.to(dev)
        poses = PoseModel([cam] * views[name], PoseConfig()) if name in views else None
        runs[name] = [TrainStep(model, dev, fused_adam=name == "fused"), cam, dict(poses=poses) if poses else {}, 0]

    def advance(run):
        step, cam, extra, count = run
        run[3] = count + 1
        step(cam, target, **extra, **(dict(view=count % extra["poses"].num_views) if extra else {}))
    for run in runs.values():                            # warm-up
        for _ in range(8):
            advance(run)
    samples = {name: [] for name in runs}
    for _block in range(max(1, args.steps // 10)):       # interleaved blocks: drift hits every run alike
        for name, run in runs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                advance(run)
            b.record()
            torch.cuda.synchronize()
            samples[name].append(a.elapsed_time(b) / 10.0)
    out = {name: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v),
                  "blocks_of_10": len(v)} for name, v in samples.items()}
    # the host's share of a pose update on an idle device: the 48-byte copy and its wait, Adam and the retraction, the
    # new camera tensor
    poses, g = runs["poses"][2]["poses"], torch.zeros(6, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        poses.step(0, g)
        poses.camera(0)
    out["poses_step_and_camera_on_an_idle_device_us"] = (time.perf_counter() - t0) / 200 * 1e6
    med = {k: out[k]["ms_per_step_median"] for k in runs}
    out["unfused_adam_ms"] = med["two_launch"] - med["fused"]
    out["pose_update_ms"] = med["poses"] - med["two_launch"]
    out["pose_update_one_view_ms"] = med["poses_one_view"] - med["two_launch"]
    return out


def main(argv=None):
    args = parse(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd import _lib
    stamp = _lib.LIB_PATH.with_suffix(_lib.LIB_PATH.suffix + ".flags")
    flags = sorted({f for f in stamp.read_text().split() if f.startswith("-DTS_")}) if stamp.exists() else []
    result = {"gaussians": args.gaussians, "image": [args.height, args.width], "blocks": args.blocks, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "library_flags": flags, "kernel": time_kernel(args)}
    if args.steps > 0:
        result["train_step"] = time_train_step(args)
    text = json.dumps(result, indent=1)
    print(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
