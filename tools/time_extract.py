#!/usr/bin/env python
"""Times the level-set surface extraction (tinysplat_amd.extract) with device events after a warm-up; prints one JSON
line per measurement (ms).

  * ``extract_surface_points``: the whole extraction, N Gaussians, the rays split over the cameras at 1920 x 1080,
    with its peak memory over the model;
  * its parts, per entry of the C ABI (``ops.kernel_timer``: events around every launch) and the render;
  * ``ts_knn grid build``: one call with no queries - what every chunk pays again - and its share of the extraction;
  * ``baseline``: the same arithmetic composed from what the package offered before (``knn_points`` plus torch ops
    restating ``density_function`` and the crossing), chunked to the same memory cap.

  ``--scene sheet`` times a surface-aligned scene instead of ``make_scene``'s volume cloud.

    python tools/time_extract.py [--scene volume|sheet] [--n 1000000] [--rays 2000000] [--cameras 4] [--reps 3] [--out time_extract.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tinysplat_amd import GaussianRasterizer, _lib, knn_points  # noqa: E402
from tinysplat_amd.extract import ExtractConfig, _camera_host, extract_surface_points, pack_model  # noqa: E402
from tinysplat_amd.ops import _ptr, _stream, kernel_timer  # noqa: E402
from tinysplat_amd.synthetic import PinholeCamera, make_scene  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def quat_to_rot(q):
    w, x, y, z = torch.unbind(F.normalize(q, dim=-1), dim=-1)
    return torch.stack([
        torch.stack([1 - 2 * (y ** 2 + z ** 2), 2 * (x * y - w * z), 2 * (x * z + w * y)], dim=-1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x ** 2 + z ** 2), 2 * (y * z - w * x)], dim=-1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x ** 2 + y ** 2)], dim=-1)], dim=-2)


@torch.no_grad()
def baseline_camera(model, cam, depth, ids, cfg, sigma_inv, sig):
    """model_gaussian.py:416-459 in torch ops on ``knn_points``, in chunks of rays that keep the chunk's tensors (the
    gathered 3 x 3 matrices dominate: 16 x 36 B per sample) under the cap."""
    h, w = depth.shape
    s = cfg.num_steps
    per_ray = s * (16 * (36 + 12 + 12 + 4 + 4 + 8 + 4) + 12) + 64
    rays = max(1, int(cfg.max_workspace_bytes) // per_ray)
    inv = torch.tensor(list(_camera_host(cam))[:16], device=DEV).view(4, 4)
    pos = torch.tensor(list(_camera_host(cam))[16:19], device=DEV)
    p22, p23 = float(cam.proj_matrix[2, 2]), float(cam.proj_matrix[2, 3])
    lin = torch.linspace(-cfg.extent_sigmas, cfg.extent_sigmas, s, device=DEV)
    es = torch.exp(model.scales)
    out = []
    for r0 in range(0, ids.shape[0], rays):
        f = ids[r0:r0 + rays]
        z = depth.reshape(-1)[f]
        ok = z > 0
        zs = torch.where(ok, z, torch.ones_like(z))
        x, y = (f % h).float(), (f // h).float()
        ndc = torch.stack(((x + 0.5 - w // 2) / h * 2, (y + 0.5 - h // 2) / w * 2, (p22 * zs + p23) / zs,
                           torch.ones_like(zs)), -1) @ inv.T
        pw = ndc[:, :3] / ndc[:, 3:4]
        ok = ok & torch.isfinite(pw).all(-1)
        pw = torch.where(ok[:, None], pw, pos.expand_as(pw)).contiguous()
        nn0 = knn_points(pw, model.means, 16)[1][:, 0]
        p_range = lin[None, :] * es[nn0].norm(dim=-1)[:, None]
        dirs = F.normalize(pw - pos, dim=-1)
        smp = (pw[:, None, :] + p_range[..., None] * dirs[:, None, :]).reshape(-1, 3).contiguous()
        nbr = knn_points(smp, model.means, 16)[1]
        mu = (smp[:, None] - model.means[nbr])[:, :, None, :]
        q = (torch.matmul(mu, sigma_inv[nbr]) * mu).sum(-1).clamp(min=0, max=1e8)
        d = torch.sum(torch.exp(-0.5 * q).squeeze(-1) * sig[nbr], dim=-1)
        d = torch.where(d > 1, torch.ones_like(d), d).reshape(-1, s)
        first = (d > cfg.surface_level).max(dim=-1, keepdim=True)[1]
        keep = ok & (d[:, 0] < cfg.surface_level) & (first[:, 0] != 0)
        fb = (first - 1).clamp(min=0)
        d_b, d_a = d.gather(1, fb)[:, 0], d.gather(1, first)[:, 0]
        t_b, t_a = p_range.gather(1, fb)[:, 0], p_range.gather(1, first)[:, 0]
        t = (cfg.surface_level - d_b) / (d_a - d_b) * (t_a - t_b) + t_b
        out.append((pw + t[:, None] * dirs)[keep])
    return torch.cat(out)


def sheet_scene(n, w, h, seed=0):
    """A surface-aligned scene, what the SuGaR terms train towards: n opaque Gaussians flattened onto the wavy sheet
    z = 5 + 0.3 sin x cos y that fills the view, tangential scale 1.25 x their spacing, normal scale a quarter of
    that.  (``make_scene``'s cloud fills a volume: its depth render sits on the cloud's front face, where a fifth of
    the ray samples find fewer than 16 means within ``ts_knn``'s five rings of cells and take its brute-force pass.)"""
    g = torch.Generator().manual_seed(seed)
    half_x, half_y = 5.3 * 1.1 * (w / 2) / (w / (2 * np.tan(np.radians(30.0)))), 0.0
    half_y = half_x * h / w
    xy = (2 * torch.rand(n, 2, generator=g) - 1) * torch.tensor([half_x, half_y])
    z = 5.0 + 0.3 * torch.sin(xy[:, 0]) * torch.cos(xy[:, 1])
    spacing = float(np.sqrt(4 * half_x * half_y / n))
    scales = torch.log(torch.cat((spacing * (1.0 + 0.5 * torch.rand(n, 2, generator=g)),
                                  spacing * (0.25 + 0.1 * torch.rand(n, 1, generator=g))), 1))
    quats = torch.cat((torch.ones(n, 1), 0.05 * torch.randn(n, 3, generator=g)), 1)
    from tinysplat_amd.synthetic import SplatModel
    return SplatModel(torch.cat((xy, z[:, None]), 1).float().contiguous(), torch.randn(n, 3, generator=g),
                      torch.zeros(n, 0, 3), scales.float(), quats, 2.0 + 0.5 * torch.randn(n, 1, generator=g), 0,
                      background=torch.zeros(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", choices=("volume", "sheet"), default="volume")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    rows = []

    def emit(call, ms, **kw):
        rows.append({"call": call, "ms": round(ms, 4), **kw})
        print(json.dumps(rows[-1]), flush=True)

    w, h = 1920, 1080
    if args.scene == "volume":
        model, _ = make_scene(args.n, 0, w, h, seed=0, scale_mult=4.0, opacity_logit_mean=2.0)
    else:
        model = sheet_scene(args.n, w, h)
    model = model.to(DEV)
    cams = []
    for i in range(args.cameras):
        pos = (0.05 * i, -0.03 * i, 0.0)
        cam = PinholeCamera.look_at_origin_plus_z(w, h, position=pos)
        cam.position = np.asarray(pos, dtype=np.float64)
        cams.append(cam)
    cfg = ExtractConfig(num_total_points=args.rays)
    shape = dict(scene=args.scene, n=args.n, rays=args.rays, cameras=args.cameras, width=w, height=h)

    def run():
        return extract_surface_points(model, cams, cfg, device=DEV, generator=torch.Generator().manual_seed(1))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    total = timed(run, args.reps)
    peak = torch.cuda.max_memory_allocated() - base
    pts = run()
    emit("extract_surface_points", total, points=int(pts.points.shape[0]), peak_mib=round(peak / 2 ** 20, 1),
         cap_mib=cfg.max_workspace_bytes >> 20, **shape)
    kernel_timer.start()
    run()
    parts = kernel_timer.stop()
    for name, (launches, mean_ms) in sorted(parts.items()):
        emit("part " + name, launches * mean_ms, launches=launches, **shape)
    with torch.no_grad():
        render = GaussianRasterizer(model, cams, device=torch.device(DEV))
        emit("part render (per camera)", timed(lambda: render(cams[0]), 5), **shape)
    lib = _lib.load()
    ws = torch.empty(int(lib.ts_knn_ws_bytes(args.n, 0, 16)), dtype=torch.uint8, device=DEV)
    means = model.means.contiguous()

    def build_only():
        lib.ts_knn(args.n, _ptr(means), 0, None, 16, None, None, _ptr(ws), None, _stream(torch.device(DEV)))
    build = timed(build_only, 20, warm=3)
    calls = parts.get("ts_knn", (0, 0.0))[0]
    emit("ts_knn grid build", build, calls_per_extraction=calls,
         share_of_extraction=round(calls * build / total, 4), **shape)
    emit("pack_model", timed(lambda: pack_model(model), 10), n=args.n)
    if not args.no_baseline:
        with torch.no_grad():
            R = quat_to_rot(model.quats)
            sigma_inv = R @ (R.transpose(-2, -1) * torch.exp(-2 * model.scales).unsqueeze(2))
            sig = torch.sigmoid(model.opacities).squeeze(-1)
            per = args.rays // args.cameras
            g = torch.Generator().manual_seed(1)
            jobs = []
            for cam in cams:
                depth = render(cam)[1]["depth"].clone()
                jobs.append((cam, depth, torch.randperm(h * w, generator=g)[:per].to(DEV)))
            baseline_camera(model, jobs[0][0], jobs[0][1], jobs[0][2][:20000], cfg, sigma_inv, sig)    # warm-up
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            runs = []
            for _ in range(args.baseline_reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                count = sum(int(baseline_camera(model, c, d, i, cfg, sigma_inv, sig).shape[0]) for c, d, i in jobs)
                b.record()
                torch.cuda.synchronize()
                runs.append(a.elapsed_time(b))
            ms = sum(runs) / len(runs)
            # the baseline covers back-projection to intersection only; the figure it is divided by also holds the
            # renders, the CPU randperm and the normals: the ratio understates the new path's advantage
            emit("baseline (knn_points + torch ops, march only)", ms, points=count, runs_ms=[round(r, 1) for r in runs],
                 peak_mib=round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1),
                 baseline_march_only_over_whole_extraction=round(ms / total, 2), **shape)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
