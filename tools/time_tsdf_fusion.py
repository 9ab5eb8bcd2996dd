#!/usr/bin/env python
"""Times the depth-map fusion on a synthetic scene.

    python tools/time_tsdf_fusion.py --cameras 200 --width 1920 --height 1080 --resolution 256 512 [--out FILE]

The scene is the unit sphere, seen by ``--cameras`` cameras spread over a sphere of radius ``--distance`` around it; every depth map is
the analytic ray-sphere depth, made on the device.  Timed with the maps and the camera table already on the device, host
clock around synchronised calls, best of ``--repeats`` after a warm-up, per resolution: ``ts_tsdf_mark``;
``ts_tsdf_integrate`` over all active bricks and all cameras in one launch, with the frustum cull on and off; the field;
count + emit; and ``fuse_depth_maps`` as a whole.  For the integration also the (corner, camera) pairs it projects (every
corner of a brick for every camera the brick's sphere test lets through, counted by a double restatement of that test),
the time per pair, and the bytes it must move - the sums and counts in and out, 24 B per corner, and one 4 B depth read
per projected pair at most - against 8 TB/s.
"""
import argparse
import ctypes
import math
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_BYTES_PER_S = 8e12


def sphere_depth(view, proj, width, height, dev):
    """The analytic depth of the unit sphere, float32 [H,W] on ``dev`` (0 where the ray misses)."""
    import torch
    v = torch.from_numpy(view.astype("float64")).to(dev)
    nx = (torch.arange(width, device=dev, dtype=torch.float64) + 0.5 - 0.5 * width) * 2.0 / width / float(proj[0, 0])
    ny = (torch.arange(height, device=dev, dtype=torch.float64) + 0.5 - 0.5 * height) * 2.0 / height / float(proj[1, 1])
    d = torch.stack(torch.broadcast_tensors(nx[None, :], ny[:, None], torch.ones((), device=dev, dtype=torch.float64)), -1)
    d = d @ v[:3, :3]
    o = -(v[:3, :3].T @ v[:3, 3])
    a, b, c = (d * d).sum(-1), 2.0 * (d @ o), (o @ o) - 1.0
    disc = b * b - 4 * a * c
    z = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
    return torch.where((disc > 0) & (z > 0), z, torch.zeros_like(z)).float().contiguous()


def projected_pairs(table_host, active, bricks, znear):
    """(pairs with the cull, pairs without): a double restatement of csrc/tsdf_math.h's sphere test per (brick, camera) of
    the ``active`` bricks of the ``BrickGrid`` ``bricks``."""
    import numpy as np
    from tinysplat_amd import _lib
    from tinysplat_amd._bricks import BRICK
    glo, h, cells, nb = bricks.lo, bricks.h, bricks.cells, bricks.bricks
    b = np.stack((active % nb[0], (active // nb[0]) % nb[1], active // (nb[0] * nb[1])), -1)
    i0 = b * BRICK
    i1 = np.minimum(i0 + BRICK, np.asarray(cells)[None, :])
    p0, p1 = np.asarray(glo)[None, :] + i0 * h, np.asarray(glo)[None, :] + i1 * h
    centre = 0.5 * (p0 + p1)
    radius = np.linalg.norm(0.5 * (p1 - p0), axis=1) + 0.0625 * h
    live = np.prod(i1 - i0 + 1, axis=1)
    recs = (_lib.TsTsdfCamera * (len(table_host) // ctypes.sizeof(_lib.TsTsdfCamera))).from_buffer_copy(table_host.tobytes())
    slack = 2.0 ** -14
    kept = np.zeros(active.shape[0], dtype=np.int64)
    for rec in recs:
        pl = np.asarray(rec.planes[:], dtype=np.float64).reshape(6, 5)
        at = centre @ pl[:, :3].T + pl[:, 3]                                    # [A,6]
        mag = np.abs(centre) @ np.abs(pl[:, :3]).T + np.abs(pl[:, 3]) + radius[:, None] * pl[:, 4]
        top, low = at + radius[:, None] * pl[:, 4], at - radius[:, None] * pl[:, 4]
        behind = top[:, 0] < znear - slack * (mag[:, 0] + abs(znear))
        side = (low[:, 1] > slack * mag[:, 1]) & (top[:, 2:] < -slack * mag[:, 2:]).any(1)
        kept += ~(behind | side)
    return int((kept * live).sum()), int(live.sum()) * len(recs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cameras", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resolution", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--fov-x", type=float, default=50.0)
    ap.add_argument("--distance", type=float, default=3.0,
                    help="of the cameras from the sphere's centre (3 with 50 degrees: every camera sees the whole sphere; "
                         "1.6 with 35 degrees: a cap each, most bricks outside most frusta)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--out", type=str, default=None, help="also write the report here")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import tsdf_cases as TC
    from tinysplat_amd import FusionConfig, _lib, fuse_depth_maps, fusion
    from tinysplat_amd._bricks import BRICK_CORNERS, BrickGrid, count_and_emit
    dev = args.device
    lib = _lib.load()
    cams, depths = [], []
    golden = math.pi * (3.0 - math.sqrt(5.0))
    for i in range(args.cameras):                              # a Fibonacci lattice on the sphere of that radius
        y = 1.0 - 2.0 * (i + 0.5) / args.cameras
        r = math.sqrt(1.0 - y * y)
        p = tuple(args.distance * v for v in (r * math.cos(golden * i), y, r * math.sin(golden * i)))
        view, proj = TC.look_at(p, (0.0, 0.0, 0.0), args.width, args.height, args.fov_x, up=(0.13, 1.0, 0.29))
        cams.append(SimpleNamespace(view_matrix=torch.from_numpy(view), proj_matrix=torch.from_numpy(proj), width=args.width,
                                    height=args.height))
        depths.append(sphere_depth(view, proj, args.width, args.height, dev))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        times, out = [], None
        for _ in range(args.repeats + 1):                      # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times[1:]), out
    say(f"{args.cameras} cameras at {args.width}x{args.height}, {args.distance} from the unit sphere's centre, fov {args.fov_x}, best of {args.repeats} (host clock, synchronised)")
    bounds = ((-1.3, -1.3, -1.3), (1.3, 1.3, 1.3))
    table_host = fusion.camera_table(cams, depths)
    table = torch.from_numpy(table_host).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    for res in args.resolution:
        cfg = FusionConfig(resolution=res, bounds=bounds, max_workspace_bytes=4 << 30)
        bricks = BrickGrid(*bounds, res, cfg.max_workspace_bytes)
        cells, total = bricks.cells, bricks.total_bricks
        trunc = ctypes.c_float(cfg.trunc_voxels * bricks.h).value
        grid, cells_c = bricks.grid_host, bricks.cells_host
        flags = torch.zeros((total,), dtype=torch.uint8, device=dev)

        def mark():
            flags.zero_()
            _lib.check(lib.ts_tsdf_mark(len(cams), table.data_ptr(), args.width * args.height, grid, cells_c, trunc, math.inf,
                                        flags.data_ptr(), s), "ts_tsdf_mark")
        t_mark, _ = timed(mark)
        active = torch.nonzero(flags).view(-1)
        a = int(active.shape[0])
        q = a * BRICK_CORNERS
        acc = torch.zeros((q,), dtype=torch.float64, device=dev)
        cnt = torch.zeros((q,), dtype=torch.int32, device=dev)
        field = torch.empty((q,), dtype=torch.float32, device=dev)

        def integrate(flag):
            acc.zero_()
            cnt.zero_()
            _lib.check(lib.ts_tsdf_integrate(a, active.data_ptr(), grid, cells_c, table.data_ptr(), 0, len(cams), trunc,
                                             cfg.znear, math.inf, flag, acc.data_ptr(), cnt.data_ptr(), s), "ts_tsdf_integrate")
        t_zero, _ = timed(lambda: (acc.zero_(), cnt.zero_()))
        t_cull, _ = timed(lambda: integrate(0))
        t_all, _ = timed(lambda: integrate(_lib.TSDF_NO_CULL))
        t_cull, t_all = t_cull - t_zero, t_all - t_zero
        pairs_cull, pairs_all = projected_pairs(table_host, active.cpu().numpy(), bricks, cfg.znear)
        t_field, _ = timed(lambda: _lib.check(lib.ts_tsdf_field(a, acc.data_ptr(), cnt.data_ptr(), 1, field.data_ptr(), s),
                                              "ts_tsdf_field"))
        counts = torch.empty((a,), dtype=torch.int32, device=dev)
        offsets = torch.empty((a,), dtype=torch.int64, device=dev)

        def mesh():
            emitted = count_and_emit(lib, bricks, active, a, field, counts, offsets, 0.0, True, False, s)
            return emitted[0].shape[0] if emitted is not None else 0
        t_mesh, tris = timed(mesh)
        t_whole, fused = timed(lambda: fuse_depth_maps(cams, depths, cfg))
        say(f"resolution {res}: cells {tuple(cells)}, {a} of {total} bricks active, {tris} triangles, "
            f"{int(fused.vertices.shape[0])} vertices")
        say(f"  mark ({args.cameras * args.width * args.height / 1e6:.0f} M pixels)            {t_mark * 1e3:9.2f} ms")
        for label, t, pairs in (("cull on ", t_cull, pairs_cull), ("cull off", t_all, pairs_all)):
            moved = q * 24 + pairs * 4
            say(f"  integrate, {label}              {t * 1e3:9.2f} ms   {pairs / 1e9:7.3f} G pairs projected, {t / pairs * 1e12:6.2f} ps "
                f"per pair; {moved / 1e9:6.2f} GB at most -> {moved / HBM_BYTES_PER_S * 1e3:6.2f} ms at 8 TB/s "
                f"({100 * moved / HBM_BYTES_PER_S / t:4.1f} % of the roofline)")
        say(f"  field                            {t_field * 1e3:9.2f} ms")
        say(f"  count + emit                     {t_mesh * 1e3:9.2f} ms")
        say(f"  fuse_depth_maps (all of it)      {t_whole * 1e3:9.2f} ms")
        del acc, cnt, field, flags
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
