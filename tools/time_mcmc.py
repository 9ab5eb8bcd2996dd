#!/usr/bin/env python
"""Times the budgeted densifier (tinysplat_amd.mcmc) on the GPU and prints one JSON line.

    python tools/time_mcmc.py [--n 1000000] [--repeats 5] [--no-step] [--out FILE]

  noise        ts_mcmc_noise at --n Gaussians with a caller's z (68 bytes per row) and with in-kernel draws (56), timed
               with device events over 50 launches per repeat, beside ts_adam_step on the same model in the same run (28
               bytes per float: parameter, gradient and both moments read, parameter and both moments written) - the
               existing streaming kernel the rates are read against.  Rates are the algorithm's bytes over the time.
  regularisers mean_opacity + mean_scale, value and gradient
  refinement   one relocation at --n with 5 % of the rows dead, and one growth step of 5 %, host clock around a
               synchronise (they contain a host read of the dead count)
  step         the config-3 training step (1 M Gaussians, 1920x1080, RGB + depth) plain, with the densifier idle (no
               terms: fused Adam kept) and with it on (regularisers, hence the two-launch Adam, and the noise), alternated
Needs a GPU: there is no CPU path and no fallback."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _events(fn, launches, repeats, torch):
    """median and spread (min, max) over ``repeats`` of the mean time of ``launches`` back-to-back calls, in seconds"""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out)}


def _wall(fn, repeats, torch):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step comparison")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: tinysplat_amd has no CPU path")
    from tinysplat_amd.mcmc import McmcConfig, McmcDensifier, inject_noise, mean_opacity, mean_scale
    from tinysplat_amd.synthetic import make_scene
    from tinysplat_amd.training import PARAM_ORDER, Adam, TrainStep
    dev, n = "cuda:0", args.n
    w, h = 1920, 1080
    model, cam = make_scene(n, 3, w, h)
    model = model.to(dev)
    g = torch.Generator().manual_seed(1)
    res = {"n": n, "repeats": args.repeats, "launches": args.launches}

    # ---- the noise kernel beside ts_adam_step
    with torch.no_grad():
        model.opacities.copy_(torch.full((n, 1), -6.0) + torch.randn(n, 1, generator=g))      # g(1 - o) > 0 on most rows
    model.requires_grad_(True)
    z = torch.randn(n, 3, generator=g).to(dev)
    optim = Adam({nm: getattr(model, nm) for nm in PARAM_ORDER})
    for nm in PARAM_ORDER:
        getattr(model, nm).grad = torch.randn(getattr(model, nm).shape, generator=g).to(dev) * 1e-6
    floats = sum(getattr(model, nm).numel() for nm in PARAM_ORDER)
    cases = {"noise_given_z": (lambda: inject_noise(model, 1e-9, z), 68 * n),
             "noise_in_kernel": (lambda: inject_noise(model, 1e-9, None, 7, 3), 56 * n),
             "adam_step": (optim.step, 28 * floats)}
    for fn, _ in cases.values():
        for _ in range(3):
            fn()
    for name, (fn, nbytes) in cases.items():
        t = _events(fn, args.launches, args.repeats, torch)
        t.update(bytes=nbytes, bytes_per_s=nbytes / t["median_s"], bytes_per_s_min=nbytes / t["max_s"],
                 bytes_per_s_max=nbytes / t["min_s"])
        res[name] = t
    for nm in PARAM_ORDER:
        getattr(model, nm).grad = None

    # ---- the regularisers
    def regs():
        o, s = model.opacities.detach().requires_grad_(True), model.scales.detach().requires_grad_(True)
        (0.01 * mean_opacity(o) + 0.01 * mean_scale(s)).backward()
    for _ in range(3):
        regs()
    res["regularisers"] = _events(regs, 20, args.repeats, torch)

    # ---- one refinement
    def refinement(kind):
        times = []
        for r in range(args.repeats):
            m2, _ = make_scene(n, 3, w, h, seed=r)
            m2 = m2.to(dev)
            with torch.no_grad():
                m2.opacities[torch.randperm(n, generator=g)[: n // 20].to(dev)] = -8.0          # 5 % dead
            o2 = Adam({nm: getattr(m2, nm) for nm in PARAM_ORDER})
            d = McmcDensifier(m2, McmcConfig(cap_max=n if kind == "relocate" else 2 * n), generator=g)
            fn = (lambda: d.relocate(o2)) if kind == "relocate" else (lambda: d.add(o2))
            if r == 0:
                fn()                                     # warm-up on a model of its own (a refinement changes its input)
                continue
            times.append(_wall(fn, 1, torch)["median_s"])
            counts = (d.last_dead if kind == "relocate" else None, m2.means.shape[0])
        return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "dead_and_rows": counts}
    res["relocate_5pct_dead"] = refinement("relocate")
    res["add_5pct"] = refinement("add")

    # ---- the training step
    if not args.no_step:
        tgt = torch.rand(h, w, 3, generator=g).to(dev)
        tgt_d = (2 + 8 * torch.rand(h, w, generator=g)).to(dev)
        steps = {}
        for name in ("plain", "mcmc_idle", "mcmc_on"):
            m3, _ = make_scene(n, 3, w, h)
            m3 = m3.to(dev)
            st = TrainStep(m3, dev)
            cfg = {"plain": None, "mcmc_idle": McmcConfig(cap_max=n, noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0,
                                                         refine_start=10 ** 9),
                   "mcmc_on": McmcConfig(cap_max=n, refine_start=10 ** 9)}[name]
            dens = None if cfg is None else McmcDensifier(m3, cfg)
            steps[name] = (st, dens)
            for s in range(1, 4):
                st(cam, tgt, tgt_d, densifier=dens, step=s)
        times = {name: [] for name in steps}
        for r in range(args.repeats):                    # alternated: other work shares the machine
            for name, (st, dens) in steps.items():
                times[name].append(_wall(lambda: [st(cam, tgt, tgt_d, densifier=dens, step=10 + s) for s in range(10)], 1,
                                         torch)["median_s"] / 10)
        res["train_step"] = {name: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v),
                                    "fused_steps": steps[name][0].optimizer.fused_steps} for name, v in times.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
