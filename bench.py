#!/usr/bin/env python
"""bench.py - Gaussians*pixels/s of the render hot path, forward + backward (BASELINE.json metric).

One "step" = one frame of the hot path over one synthetic scene already resident in HBM:
project_gaussians -> spherical_harmonics -> clamp -> rasterize_gaussians (RGB) -> clamp, then the
backward of L = (rgb * w).sum() down to the six parameter tensors (means, log-scales, quats,
opacity logits, colors_dc, colors_rest).  Default workload = BASELINE.json configs[2]:
1 M Gaussians, SH degree 3, 1920x1080.  With --depth the depth output of the reference adapter
(rasterize.py:47-51) is rendered and differentiated too.

N > 1: one rank per GPU.  ``python bench.py --gpus N`` from a plain shell re-launches itself under
``torch.distributed.run`` (127.0.0.1 rendezvous); started by ``torch.distributed.run`` it uses the
ranks it is given.  Default design (--shard-mode gaussians): every rank owns N/G Gaussians and one stripe of tile
rows, records / gradient rows travel by two all_to_alls (sharded.py); --shard-mode replicated is the north star's
design (replicated parameters, stripes, one RCCL all-reduce of the 2-D gradient buffers, sharding.py); "both" times
the second beside the first.  A preflight collective decides before the first frame whether the sharded exchange
is usable on the node.  The total work is fixed, so scaling is "strong".

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit,
higher_is_better, dtype, ms_per_step and the workload's config).  --full adds everything else the bench measures:
the step with the loss kernels inside it, the RGB + depth frame, the per-entry kernel table and the rooflines, the PMC
passes, the read-bandwidth microbenchmark, the CPU baseline and, at N > 1, the time inside collectives and the second
shard design.  --dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (dump_outputs).

Prints ONE JSON line on rank 0 (the last line of stdout).
"""
from __future__ import annotations

import argparse
import collections
import csv
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec peak; four SIMD-32 per CU, a wave64 VALU instruction
# issues over 2 cycles ("Per-instruction cycle constants": v_fma_f32 2 cyc) = 256 CUs x 4 SIMDs x 32 lanes x
# 2.4 GHz = 78.6 T lane-operations/s = the 157.3 TFLOP/s fp32 vector peak counted as FMAs.  Measured here with
# s_memtime (tools/micro/op_bench2.hip, profiles/r04a_op_microbench2.txt): v_fma / mul / add / mov 1.94 - 1.98
# cycles with >= 4 waves per SIMD; ONE wave issues an instruction every 4.6 - 5.3 cycles whatever its
# dependencies (tools/micro/lat_bench.hip), so the rate needs >= 3 resident waves.
HBM_PEAK_GBS = 8000.0
SIMDS = 256 * 4
VALU_LANE_OPS_PEAK = SIMDS * 32 * 2.4e9
VALU_FP32_PEAK_TFLOPS = 157.3
SQ_INSTANCES = 32          # SQ_BUSY_CYCLES is summed over 8 XCDs x 4 shader engines

# C-ABI entry -> stage of SURVEY.md 8(d) D5.  "raster_bwd" is the compositing backward INCLUDING
# the reduction of the per-(tile, Gaussian) rows (D5 counts the gradient scatter in that stage), so
# the two entries are timed together when that stage is priced.
CLASS_WEIGHT = {"ts_raster_fwd": 2.71, "ts_raster_bwd": 2.55}      # pipe cycles per VALU instruction, priced ISA (round 6)
STAGE_OF = {
    "ts_project_fwd": "project_fwd", "ts_project_bwd": "project_bwd",
    "ts_sh_fwd": "sh_fwd", "ts_sh_colors_fwd": "sh_fwd",
    "ts_colors_pack_fwd": "sh_fwd",          # colour stage + record packing in one launch (frame path)
    "ts_sh_bwd": "sh_bwd", "ts_sh_colors_bwd": "sh_bwd", "ts_sh_colors_bwd_adam": "sh_bwd", "ts_project_bwd_adam": "project_bwd",
    "ts_scan_tiles": "bin_sort", "ts_bin_count": "bin_sort", "ts_tile_offsets": "bin_sort",
    "ts_bin_scatter": "bin_sort", "ts_sort_tiles": "bin_sort", "ts_pack_splats": "bin_sort",
    "ts_raster_fwd": "raster_fwd",
    "ts_raster_bwd": "raster_bwd", "ts_reduce_partials": "raster_bwd", "ts_reduce_partials_rows": "raster_bwd",
}


def stage_alg_bytes(stage: str, n: int, i: int, p: int, t: int, k: int, ch: int = 3) -> float:
    """SURVEY.md 8(d) D5, per stage and per pass, with the measured I (bounding-box pairs, the
    count gsplat's lists hold).  A 4-channel (RGB + depth) pass moves 4 more bytes per pair and
    pixel than D5's 3-channel figures in each direction."""
    extra = 4.0 * (ch - 3)
    return {
        "project_fwd": 96.0 * n,
        "sh_fwd": (24.0 + 12.0 * k) * n,
        "bin_sort": 28.0 * n + 44.0 * i + 8.0 * t,
        "raster_fwd": (40.0 + extra) * i + (20.0 + extra) * p + 8.0 * t,
        "raster_bwd": (24.0 + extra) * p + (76.0 + 2 * extra) * i + (36.0 + extra) * n,
        "sh_bwd": (24.0 + 12.0 * k) * n,
        "project_bwd": 144.0 * n,
    }[stage]


def entry_alg_bytes(entry: str, stage: str, n: int, i: int, p: int, t: int, k: int, ch: int = 3):
    """The share of its D5 stage that ONE C-ABI entry moves, where a stage has several entries; None = the stage is
    not split here (then only the stage as a whole is priced).  raster_bwd: the compositing kernel reads the pixel
    state and the pairs' records and writes the per-pair gradient rows (D5's scatter); the reduction writes the
    per-Gaussian results."""
    extra = 4.0 * (ch - 3)
    if stage == "raster_bwd":
        if entry == "ts_raster_bwd":
            return (24.0 + extra) * p + (76.0 + 2 * extra) * i
        if entry in ("ts_reduce_partials", "ts_reduce_partials_rows"):
            return (36.0 + extra) * n
    if stage in ("raster_fwd", "project_fwd", "project_bwd", "sh_fwd", "sh_bwd"):       # one entry per stage
        return stage_alg_bytes(stage, n, i, p, t, k, ch)
    return None


def frame_alg_bytes(n, i, p, t, k, depth):
    """D5's whole-frame figures.  RGB only: 736 N + 160 I + 44 P (+16 T).  With the depth output the
    reference composites twice (772 N + 276 I + 88 P); this build composites RGB + depth in ONE
    4-channel pass, so the bytes it has to move are the one-pass figure below (D5's per-stage terms
    with 4 channels), which is what is priced - not the two-pass formula."""
    if depth:
        return 748.0 * n + 172.0 * i + 52.0 * p + 16.0 * t
    return 736.0 * n + 160.0 * i + 44.0 * p + 16.0 * t


def measure_read_bandwidth(dev, gib: float = 2.0, reps: int = 10) -> float:
    """Achievable HBM read bandwidth (GB/s) of this GPU: ts_bench_stream_read over a buffer far larger
    than the 256 MiB Infinity Cache, best of `reps` (BW_read_measured)."""
    from tinysplat_amd import _lib
    lib = _lib.load()
    n = int(gib * (1 << 30)) // 4
    buf = torch.ones(n, dtype=torch.float32, device=dev)
    sink = torch.zeros(4, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    best = 0.0
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.ts_bench_stream_read(buf.data_ptr(), n, sink.data_ptr(), s), "ts_bench_stream_read")
        b.record()
        b.synchronize()
        best = max(best, 4.0 * n / (a.elapsed_time(b) * 1e-3) / 1e9)
    del buf
    return best


GATHER_CAL_RECORDS = 4_000_000       # table of 48-byte records (192 MB: beyond the L2s, inside the Infinity Cache)
GATHER_CAL_GATHERS = 8_000_000       # random record reads of the calibration launch


def run_gather_calibration(dev) -> None:
    """One launch of ts_bench_gather48 on a known record count (the PMC passes read its FETCH_SIZE)."""
    from tinysplat_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(7)
    table = torch.ones((GATHER_CAL_RECORDS, 12), dtype=torch.float32, device=dev)
    ids = torch.randint(0, GATHER_CAL_RECORDS, (GATHER_CAL_GATHERS,), generator=g, dtype=torch.int32).to(dev)
    sink = torch.zeros(4, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(2):
        _lib.check(lib.ts_bench_gather48(table.data_ptr(), ids.data_ptr(), GATHER_CAL_GATHERS, sink.data_ptr(), s),
                   "ts_bench_gather48")
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------
# CPU baseline: the oracle on the host cores, beside the GPU number
# --------------------------------------------------------------------------------------------------
def _cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def cpu_baseline(budget_s: float = 100.0):
    """D6: the pure-PyTorch CPU oracle (kind "port") driven through the adapter's recipe, 2 warm-ups,
    median of up to 5 runs, everything under a wall-clock budget:

      * BASELINE config 1 (10 k Gaussians, SH 0, 256x256, forward RGB) with
        ``torch.set_num_threads(<all available cores>)`` as D6 states, and again with 16 threads (the
        oracle is thousands of small tensor ops; on a many-core host the thread-pool hand-off costs
        more than it buys) - the faster setting is used for config 2 and both are reported;
      * BASELINE config 2 (100 k, SH 3, 1920x1080, fwd+bwd RGB): first on a bounded sample - the
        same scene, camera and resolution, compositing only tile rows 30..37 of 68 (11.9 % of the
        pixels; projection and SH for all N, as one rank of a sharded frame would) - and, when the
        full frame is predicted to fit the remaining budget, on the whole frame.

    ``value`` is the config-2 figure (full frame when measured, else the sample) in
    Gaussians*pixels/s = N * pixels composited / median time.
    """
    from oracle import gsplat_oracle as O
    from tinysplat_amd.rasterizer import project_args, raster_args, sh_args
    from tinysplat_amd.synthetic import loss_weights, make_scene
    t_begin = time.perf_counter()
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cpu = _cpu_model()

    def timed(fn, warm=2, runs=5, max_seconds=None):
        """-> (median seconds, timed runs).  Stops as soon as `max_seconds` have passed (checked after
        every call, warm-ups included); if not even one timed run fitted, the last warm-up stands in
        and the run count is reported as 0."""
        t_in = time.perf_counter()
        ts, last = [], None
        for i in range(warm + runs):
            t0 = time.perf_counter()
            fn()
            last = time.perf_counter() - t0
            if i >= warm:
                ts.append(last)
            if max_seconds is not None and time.perf_counter() - t_in > max_seconds:
                break
        return (_median(ts), len(ts)) if ts else (last, 0)

    # config 1: forward only
    n1, w1, h1 = 10_000, 256, 256
    m1, c1 = make_scene(n1, 0, w1, h1, seed=0)

    def fwd1():
        with torch.no_grad():
            xys, depths, radii, conics, nth, _ = O.project_gaussians(*project_args(m1, c1, (w1, h1), "cpu"))
            col = torch.clamp(O.spherical_harmonics(*sh_args(m1, c1, "cpu")) + 0.5, min=0.0)
            O.rasterize_gaussians(*raster_args(m1, xys, depths, radii, conics, nth, col, (w1, h1)))

    config1 = {"workload": "BASELINE configs[0]: 10k Gaussians, SH 0, 256x256, forward RGB"}
    best_t, cores = None, avail
    for th in sorted({avail, min(16, avail)}, reverse=True):
        torch.set_num_threads(th)
        t1, r1 = timed(fwd1, max_seconds=0.08 * budget_s)
        config1[f"threads_{th}"] = {"value": n1 * w1 * h1 / t1, "ms_per_frame": t1 * 1e3, "runs": r1}
        if best_t is None or t1 < best_t:
            best_t, cores = t1, th
    torch.set_num_threads(cores)
    config1["value"] = n1 * w1 * h1 / best_t

    # config 2: fwd+bwd, bounded sample (a stripe of tile rows), then the full frame if affordable
    n2, w2, h2, sh2 = 100_000, 1920, 1080, 3
    m2, c2 = make_scene(n2, sh2, w2, h2, seed=0)
    m2.requires_grad_(True)
    w_rgb, _ = loss_weights(w2, h2)
    tby = (h2 + 15) // 16

    def fwd_bwd2(rows):
        def run():
            for p_ in m2.parameters():
                p_.grad = None
            xys, depths, radii, conics, nth, _ = O.project_gaussians(*project_args(m2, c2, (w2, h2), "cpu"))
            col = torch.clamp(O.spherical_harmonics(*sh_args(m2, c2, "cpu")) + 0.5, min=0.0)
            ra = raster_args(m2, xys, depths, radii, conics, nth, col, (w2, h2))
            img, _ = O.rasterize_gaussians(*ra, tile_rows=None if rows == (0, tby) else rows)
            y0 = 16 * rows[0]
            (torch.clamp(img, max=1.0) * w_rgb[y0:y0 + img.shape[0]]).sum().backward()
        return run

    rows = (30, 38)
    ts, rs = timed(fwd_bwd2(rows), max_seconds=0.3 * budget_s)
    px_s = (min(16 * rows[1], h2) - 16 * rows[0]) * w2
    sample = {"value": n2 * px_s / ts, "ms": ts * 1e3, "runs": rs, "pixels": px_s,
              "workload": f"BASELINE configs[1] (100k Gaussians, SH 3, 1920x1080, fwd+bwd RGB), tile rows "
                          f"{rows[0]}..{rows[1] - 1} of {tby} only ({100.0 * px_s / (w2 * h2):.1f} % of the pixels)"}
    out = {"value": sample["value"], "unit": "Gaussians*pixels/s", "cores": cores, "cores_available": avail,
           "kind": "port", "cpu": cpu, "config1_fwd": config1, "config2_sample": sample}
    est_full = ts * (w2 * h2) / px_s
    left = budget_s - (time.perf_counter() - t_begin)
    if 4.0 * est_full <= left:           # 2 warm-ups + >= 2 timed runs fit
        tf, rf = timed(fwd_bwd2((0, tby)), max_seconds=left)
        out["config2_full"] = {"value": n2 * w2 * h2 / tf, "ms_per_frame": tf * 1e3, "runs": rf}
        out["value"] = out["config2_full"]["value"]
        what = f"whole frame, median of {rf} runs = {tf * 1e3:.0f} ms/frame"
    else:
        what = (f"bounded sample: tile rows {rows[0]}..{rows[1] - 1} of {tby}, median of {rs} runs = "
                f"{ts * 1e3:.0f} ms (whole frame predicted {est_full:.1f} s/frame: 2 warm-ups + runs do not fit "
                f"the {budget_s:.0f} s budget)")
    out["sample"] = (f"oracle (pure PyTorch, CPU) through the adapter recipe on {cores} of {avail} threads of {cpu}; "
                     f"BASELINE configs[1] 100k SH3 1920x1080 fwd+bwd RGB, {what}; configs[0] forward "
                     f"{best_t * 1e3:.0f} ms/frame = {config1['value']:.3g} G*px/s; 2 warm-ups each")
    return out


def cpu_baseline_guarded(timeout_s: float = 240.0):
    """Runs cpu_baseline() in a child process so that a pathological host (thread-pool stalls) can
    never hang the bench: on a timeout the bench line carries an explanatory stub instead."""
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--cpu-baseline-only"],
                           capture_output=True, text=True, timeout=timeout_s)
        line = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        if r.returncode == 0 and line:
            return json.loads(line[-1])
        return {"value": None, "unit": "Gaussians*pixels/s", "cores": 0, "kind": "port",
                "sample": f"cpu_baseline child failed (rc {r.returncode}): {r.stderr[-300:]}"}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "Gaussians*pixels/s", "cores": 0, "kind": "port",
                "sample": f"cpu_baseline child exceeded {timeout_s:.0f} s and was stopped"}


# --------------------------------------------------------------------------------------------------
# PMC counters of the same workload (rocprofv3, one counter group per pass, no tracing)
# --------------------------------------------------------------------------------------------------
KERNEL_TO_ENTRY = [("raster_bwd_kernel", "ts_raster_bwd"), ("raster_fwd_kernel", "ts_raster_fwd"),
                   ("reduce_partials_kernel", "ts_reduce_partials"), ("sort_tiles", "ts_sort_tiles"),
                   ("bin_scatter_", "ts_bin_scatter"), ("bin_count_kernel", "ts_bin_count"),
                   ("sh_colors_fwd_kernel", "ts_colors_pack_fwd"), ("sh_colors_fwd_sparse_kernel", "ts_colors_pack_fwd"),
                   ("sh_colors_bwd_kernel", "ts_sh_colors_bwd"),
                   ("project_fwd_kernel", "ts_project_fwd"), ("project_bwd_kernel", "ts_project_bwd"),
                   ("pack_splats_kernel", "ts_pack_splats"), ("gather48_kernel", "gather48_calibration"),
                   ("column_scan_kernel", "ts_tile_offsets"), ("tile_offsets_kernel", "ts_tile_offsets"),
                   ("scan_local_kernel", "ts_scan_tiles"), ("scan_add_kernel", "ts_scan_tiles"),
                   ("route_count_kernel", "ts_route_count"), ("route_scan_kernel", "ts_route_count"),
                   ("route_pack_kernel", "ts_route_pack"), ("route_accumulate_kernel", "ts_route_accumulate"),
                   ("import_records_kernel", "ts_import_records"), ("import_pack_kernel", "ts_import_pack")]


def collect_pmc(workload_argv, timeout_s: float = 150.0):
    """Re-runs a few frames of THIS workload under ``rocprofv3 --pmc`` - FETCH_SIZE, WRITE_SIZE,
    SQ_INSTS_VALU and the SQ activity counters in separate passes, never combined with tracing
    (MI355X_MICROARCH.md, HBM section) - and returns {entry: {"fetch_kib", "write_kib", "valu_insts",
    "valu_active_quads", "sq_busy_cycles", "wave_quads"}} as means per dispatch, or None when rocprofv3 is
    unavailable / a pass fails (the caller then falls back to ``profiles/``)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    res = collections.defaultdict(dict)
    for counters, keys in ((("FETCH_SIZE",), ("fetch_kib",)), (("WRITE_SIZE",), ("write_kib",)),
                           (("SQ_INSTS_VALU",), ("valu_insts",)),
                           (("SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES"),
                            ("valu_active_quads", "sq_busy_cycles", "wave_quads"))):
        tmp = tempfile.mkdtemp(prefix="ts_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--pmc", *counters, "--output-format", "csv", "-d", tmp, "-o", "pmc", "--",
                   sys.executable, str(ROOT / "bench.py"), "--steps", "2", "--warmup", "1",
                   "--profile-steps", "1", "--no-cpu-baseline", "--no-pmc", "--no-bandwidth",
                   "--gather-calibration", "--no-rgbd-figure", "--full"] + workload_argv
            env = dict(os.environ, TMPDIR="/tmp")
            for k_ in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
                env.pop(k_, None)
            r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                               timeout=timeout_s)
            files = list(Path(tmp).rglob("*counter_collection.csv"))
            if r.returncode != 0 or not files:
                return None
            # per KERNEL means first, then summed per entry: an entry that launches several kernels per call
            # (sort, scan, offsets, the two scatter hops) is the sum of its kernels' per-dispatch means
            key_of = dict(zip(counters, keys))
            acc, seen = collections.defaultdict(float), collections.defaultdict(set)
            for row in csv.DictReader(open(files[0])):
                key = key_of.get(row["Counter_Name"])
                if key is None:
                    continue
                name = row["Kernel_Name"]
                entry = next((e for pat, e in KERNEL_TO_ENTRY if pat in name), None)
                if entry is None:
                    continue
                acc[(entry, name, key)] += float(row["Counter_Value"])
                seen[(entry, name, key)].add(row["Dispatch_Id"])
            per_entry_sum = collections.defaultdict(float)
            for (entry, name, key), tot in acc.items():
                per_entry_sum[(entry, key)] += tot / max(1, len(seen[(entry, name, key)]))
            for (entry, key), v in per_entry_sum.items():
                res[entry][key] = v
                if entry == "ts_reduce_partials":        # the sharded frame calls the same kernel through _rows
                    res["ts_reduce_partials_rows"][key] = v
        except Exception:
            return None
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return dict(res)


DUMP_BUDGET_BYTES = 60 << 20          # --dump-outputs: all files of one run together (headers aside)
DUMP_SEED = 12345


def dump_outputs(out_dir, arrays) -> None:
    """Writes every tensor of `arrays` ({name: tensor}) as out_dir/<name>.npy, float64 as float64, everything else
    as float32.  Tensors that together exceed DUMP_BUDGET_BYTES are cut down: the budget is shared out evenly, the
    smaller tensors are written whole and each larger one as a 1-D sample of its flattened entries at indices drawn
    from a generator seeded with DUMP_SEED and the tensor's size (sorted, repeats dropped) - the same entries in every
    run with the same arguments, so that two builds can be compared output for output."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    items = sorted(arrays.items(), key=lambda kv: kv[1].numel())
    left = DUMP_BUDGET_BYTES
    for i, (name, t) in enumerate(items):
        t = t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32)
        take = min(t.numel(), left // (len(items) - i) // t.element_size())
        left -= take * t.element_size()
        if take < t.numel():
            g = torch.Generator(device="cpu").manual_seed(DUMP_SEED + t.numel())
            idx = torch.randint(0, t.numel(), (take,), generator=g).unique()
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(out_dir / f"{name}.npy", t.cpu().numpy())


def _log(msg: str) -> None:
    """Progress on stderr (stdout carries the one JSON line)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def bind_to_gpu_numa_node(index):
    """One process per GPU, on the cores of the GPU's own NUMA node (sysfs local_cpulist of its PCI function): the
    boxes have two sockets, the scheduler moves an unpinned process between them, and a frame of a small scene
    is a chain of doorbell writes and one spin on a mapped host word (config 2: 0.29 - 0.30 ms pinned,
    0.30 - 0.39 ms unpinned).  -> the cpulist string, or None when sysfs does not say / the mask cannot be set."""
    try:
        p = torch.cuda.get_device_properties(index)
        bus = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        text = Path(f"/sys/bus/pci/devices/{bus}/local_cpulist").read_text().strip()
        cpus = set()
        for part in text.split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return text
    except (OSError, ValueError, AttributeError, RuntimeError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", "--gaussians", dest="n", type=int, default=1_000_000,
                    help="(--gaussians: the spelling to use behind torch.distributed.run, whose own parser takes --n for an "
                         "ambiguous abbreviation of --nnodes / --nproc-per-node)")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scale-mult", type=float, default=1.0)
    ap.add_argument("--depth", action="store_true", help="also render and differentiate the depth output")
    ap.add_argument("--spatial-sort", action="store_true",
                    help="reorder the synthetic scene along a Morton curve of the means before it is rendered "
                         "(SplatModel.spatial_sort_: same scene, different memory order; outside the timed region)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true",
                    help="do not re-run the workload under rocprofv3 --pmc for roofline.traffic / valu_roofline")
    ap.add_argument("--no-bandwidth", action="store_true", help="skip the read-bandwidth microbenchmark")
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--train-step", action="store_true",
                    help="time the whole training step of SURVEY 8(f) F1 instead: render RGB+depth, "
                         "L1 + DSSIM (+ depth L1) loss, backward, Adam (single GPU)")
    ap.add_argument("--forward-only", action="store_true",
                    help="time the no_grad forward frame only (the viewer path, SURVEY 8(f) F4)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group and run the gradient all-reduce even with one rank")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL)")
    ap.add_argument("--shard-mode", default=None, choices=("gaussians", "replicated", "both"),
                    help="default: 'both' with more than one rank and --full (so that a scaling run measures the north "
                         "star's stripes + all-reduce design beside the Gaussian-sharded one), 'gaussians' otherwise.  "
                         "N > 1 (and --emulate-ranks): 'gaussians' = every rank owns N/G Gaussians and one stripe, "
                         "records / gradient rows travel by all_to_all (sharded.py); 'replicated' = the north star's "
                         "design: parameters on every rank, tile-row stripes, one dense all-reduce of the 2-D "
                         "gradients (sharding.py); 'both' = time the second beside the first (sub-record "
                         "'replicated_mode' of the line)")
    ap.add_argument("--single-device", action="store_true",
                    help="functional test of the N>1 path on a 1-GPU box: every rank uses cuda:0 (use with "
                         "--backend gloo; RCCL refuses two ranks on one GPU).  Not a measurement.")
    ap.add_argument("--emulate-ranks", type=int, default=0,
                    help="single-GPU estimate of the per-rank step at this many tile-row stripes: renders "
                         "only stripe --emulate-rank of that many (with --force-dist the 1-rank all-reduce "
                         "runs too); the printed value is NOT a multi-GPU measurement")
    ap.add_argument("--emulate-rank", type=int, default=0)
    ap.add_argument("--top-third", type=float, default=0.0,
                    help="skewed scene: this share of the Gaussians lies in the top third of the image (make_scene)")
    ap.add_argument("--balance-stripes", action="store_true",
                    help="Gaussian-sharded frame: tile-row stripes balanced by the lists' work (pairs + a cost per "
                         "tile) instead of equal row counts - from the whole frame's lists with --emulate-ranks, from "
                         "the warm-up frames' own lists (all-reduced over the ranks) at N > 1")
    ap.add_argument("--config", type=int, default=None,
                    help="BASELINE.json config shortcut: 2 = 100k/1080p, 3 = 1M/1080p (default), "
                         "5 = 5M/4K with depth")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gather-calibration", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-rgbd-figure", action="store_true",
                    help="do not time the RGB + depth frame (the reference's full adapter call) beside the RGB headline")
    ap.add_argument("--upstream", default="grad", choices=("grad", "loss"),
                    help="how the backward pass of a step is started.  'grad' (default): D2's loss L = (rgb * w_rgb).sum() "
                         "(+ (depth * w_d).sum()) enters as its analytic upstream gradient, v_out = w, handed to "
                         "torch.autograd.backward - the timed step is the render path's forward + backward and nothing "
                         "else.  'loss': the loss is evaluated by torch kernels inside the step (rocBLAS dot, fill, mul: "
                         "~33 us per frame on config 3 that belong to no row of SURVEY 8(a)) - rounds 1-4 timed this")
    ap.add_argument("--prewarm-ms", type=float, default=400.0,
                    help="untimed steps run for this long BEFORE the W warm-up steps, so that the K timed steps see the GPU's "
                         "steady state: the driver's W = 5 warm-up steps are 5 ms of GPU work behind seconds of host-side "
                         "scene set-up, i.e. the timed 20 ms sat inside the clock / power ramp (round 6: 1.06 - 1.13 ms from "
                         "run to run on one box with W = 5 .. 10, 1.043 - 1.046 after 200 frames).  0 = none.  The timed "
                         "region is unchanged: exactly K steps between barrier + synchronize")
    ap.add_argument("--no-numa-bind", action="store_true",
                    help="leave the process's CPU affinity alone (default: the cores of the GPU's NUMA node)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (module docstring); the --no-cpu-baseline, "
                         "--no-pmc, --no-bandwidth, --no-rgbd-figure and --profile-steps options act on these parts")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (images, parameter gradients; "
                         "--train-step: loss terms and updated parameters) to DIR/<name>.npy, rank 0's share at N > 1")
    args = ap.parse_args()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline()), flush=True)
        return
    if args.config == 2:
        args.n = 100_000
    elif args.config == 5:
        args.n, args.width, args.height, args.depth = 5_000_000, 3840, 2160, True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.shard_mode is None:
        args.shard_mode = "both" if (world > 1 or args.gpus > 1) and args.full else "gaussians"
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher of N ranks on this node
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), str(Path(__file__).resolve())] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        raise SystemExit(subprocess.run(cmd, env=env).returncode)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    import torch.distributed as dist
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    host_cpus = None if args.no_numa_bind else bind_to_gpu_numa_node(local_rank)
    if world > 1 or args.force_dist:
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)

    from tinysplat_amd import ops
    from tinysplat_amd.rasterizer import GaussianRasterizer
    from tinysplat_amd.sharding import render_stripe
    from tinysplat_amd.synthetic import loss_weights, make_scene

    n, w, h, sh = args.n, args.width, args.height, args.sh_degree
    model, cam = make_scene(n, sh, w, h, seed=0, scale_mult=args.scale_mult, top_third=args.top_third)
    model = model.to(dev)
    if args.spatial_sort:
        model.spatial_sort_()
    model.requires_grad_(True)
    w_rgb, w_d = loss_weights(w, h)
    w_rgb, w_d = w_rgb.to(dev), w_d.to(dev)
    w_rgbd = torch.cat([w_rgb, w_d.unsqueeze(-1)], dim=-1).contiguous()       # v_out of a 4-channel stripe image

    def backprop(outs, y0=0, y1=None):
        """Backward pass of D2's loss for the outputs `outs` = [(tensor, weights)]: L = sum((t * w).sum())."""
        if args.upstream == "grad":      # dL/dt = w: the analytic upstream gradient, no loss kernels in the step
            torch.autograd.backward([t_ for t_, _ in outs], [w_[y0:y1] for _, w_ in outs])
            return
        loss = None
        for t_, w_ in outs:
            l_ = torch.dot(t_.reshape(-1), w_[y0:y1].reshape(-1))
            loss = l_ if loss is None else loss + l_
        loss.backward()

    adapter = GaussianRasterizer(model, None, device=dev)
    sharded = world > 1 or args.emulate_ranks > 1 or args.force_dist
    # ---- which multi-GPU design runs is decided BEFORE the first frame (VERDICT r3 / ADVICE r3): every rank makes
    # the same tiny all_to_all_single with uneven split sizes and the ranks agree with an all-reduce, so a backend
    # that rejects the Gaussian-sharded exchange sends all ranks to the replicated design together instead of
    # leaving some of them blocked inside a frame.
    shard_info = {"requested": args.shard_mode, "fallback": False, "preflight": None}
    mode_first = "gaussians" if args.shard_mode in ("gaussians", "both") else "replicated"
    if world > 1 and mode_first == "gaussians":
        from tinysplat_amd._comm import preflight_sharded_exchange
        ok_, err_ = preflight_sharded_exchange(dev)
        shard_info["preflight"] = "ok" if ok_ else (err_ or "failed on another rank")
        if not ok_:
            _log(f"rank {rank}: all_to_all_single with split sizes is not usable here ({err_}); replicated design")
            shard_info["fallback"] = True
            mode_first = "replicated"
    shard_info["ran"] = mode_first
    # Gaussian-sharded frame: this rank keeps only the rows it owns
    gshard = None
    if mode_first == "gaussians" and (world > 1 or args.emulate_ranks > 1) and not args.train_step \
            and not args.forward_only:
        from tinysplat_amd.sharded import (DistExchange, ReplayExchange, ShardLayout, export_records,
                                           render_sharded, shard_model)
        if world > 1:
            g_rank, g_world = rank, world
        else:
            g_rank, g_world = args.emulate_rank, args.emulate_ranks
        stripes_ = None
        if args.balance_stripes and world == 1:
            # emulation: the whole model is here - one forward frame of it gives every tile row's work
            from tinysplat_amd import frame as _fr
            from tinysplat_amd.sharded import balanced_stripes, row_work
            with torch.no_grad():
                adapter(cam, (w, h), sh)
            b_ = _fr.last_binning[dev.index]
            if b_.cam.wide_tiles:
                raise SystemExit("--balance-stripes: the probe frame used wide lists (set TS_WIDE_TILES=0)")
            stripes_ = balanced_stripes(row_work(b_.tile_bins, b_.cam.tile_bounds_x), g_world)
            _log(f"work-balanced stripes (tile rows): {stripes_}")
        layout = ShardLayout(n, g_world, g_rank, (w, h), stripes_)
        shard = shard_model(model, g_world, g_rank).requires_grad_(True)
        if world > 1:
            exchange = DistExchange()
        else:       # what the other ranks would send to this one, recorded once (outside the timed region)
            parts, counts = [], []
            for src in range(g_world):
                rec, cnt = export_records(shard_model(model, g_world, src), cam, dev, layout.for_rank(src), args.depth)
                o = sum(cnt[:g_rank])
                parts.append(rec[o:o + cnt[g_rank]].clone())
                counts.append(cnt[g_rank])
            exchange = ReplayExchange(g_rank, counts, torch.cat(parts, dim=0))
        gshard = [shard, layout, exchange]
    both_modes = args.shard_mode == "both" and gshard is not None and world > 1
    if gshard is not None and not both_modes:
        model_params = list(gshard[0].parameters())
        del model
    else:
        model_params = list(model.parameters()) + (list(gshard[0].parameters()) if gshard is not None else [])

    trainer = None
    if args.train_step:
        if world > 1:
            raise SystemExit("--train-step is a single-GPU mode")
        from tinysplat_amd.training import TrainStep
        trainer = TrainStep(model, dev)
        train_snapshot = [p_.detach().clone() for p_ in model.parameters()]     # (see the pre-warm phase of time_steps)
        g_ = torch.Generator().manual_seed(2)
        tgt_rgb = torch.rand(h, w, 3, generator=g_).to(dev)
        tgt_depth = (2.0 + 8.0 * torch.rand(h, w, generator=g_)).to(dev)

    step_mode = [mode_first]           # 'gaussians' | 'replicated': which design step() runs (N > 1)
    # --dump-outputs: what the latest step() handed to its caller besides the parameters' .grad (kept only then)
    last_out = {} if args.dump_outputs else None

    def step():
        if trainer is not None:
            res = trainer(cam, tgt_rgb, tgt_depth)
            if last_out is not None:
                last_out.update({k_: torch.as_tensor(res[k_]) for k_ in ("loss", "l1", "ssim")})
            return
        for p_ in model_params:
            p_.grad = None
        if gshard is not None and step_mode[0] == "gaussians":
            out, (y0, y1), _ = render_sharded(gshard[0], cam, dev, gshard[1], gshard[2], with_depth=args.depth)
            if last_out is not None:
                last_out["image"] = out.detach()
            backprop([(out, w_rgb if out.shape[2] == 3 else w_rgbd)], y0, y1)
            return
        if args.forward_only:
            with torch.no_grad():
                rgb, extras = adapter(cam, (w, h), sh)
            if last_out is not None:
                last_out.update(rgb=rgb, depth=extras["depth"])
            return
        if not sharded and args.depth:           # the adapter call itself (rasterize.py:26-62)
            rgb, extras = adapter(cam, (w, h), sh)
            if last_out is not None:
                last_out.update(rgb=rgb.detach(), depth=extras["depth"].detach())
            # D2's loss on both outputs, (rgb * w).sum() + (depth * w_d).sum()
            backprop([(rgb, w_rgb), (extras["depth"], w_d)])
        else:
            if args.emulate_ranks > 1 and world == 1:
                r_, ws_ = args.emulate_rank, args.emulate_ranks
            else:
                r_, ws_ = rank, world
            out, (y0, y1), _ = render_stripe(model, cam, (w, h), dev, r_, ws_, with_depth=args.depth,
                                             collective=(world > 1 or args.force_dist))
            if last_out is not None:
                last_out["image"] = out.detach()
            # D2's loss (rgb * w).sum() (+ (depth * w_d).sum() on the fourth channel)
            if out.shape[2] == 3:
                backprop([(out, w_rgb)], y0, y1)
            elif args.depth:
                backprop([(out, w_rgbd)], y0, y1)
            else:                        # a 4-channel stripe whose depth takes no part in the loss
                (out[:, :, :3] * w_rgb[y0:y1]).sum().backward()

    def barrier():
        if world > 1 or args.force_dist:
            dist.barrier()
        torch.cuda.synchronize()

    if rank == 0:
        _log(f"scene ready (N={n}, {w}x{h}); warm-up")

    def time_steps():
        """W warm-up steps, then exactly K steps between barrier + synchronize on both sides -> (max over ranks of
        the wall time, every rank's own time)."""
        if args.prewarm_ms > 0:          # steady state first (clocks, allocator pools): untimed, see --prewarm-ms
            for _ in range(4):           # (the first steps carry first-use costs - hundreds of ms: not a step time)
                step()
            torch.cuda.synchronize()
            t_pw = time.perf_counter()
            for _ in range(4):
                step()
            torch.cuda.synchronize()
            est = (time.perf_counter() - t_pw) / 4
            if world > 1:                # every rank must run the SAME number of steps (they hold collectives)
                tt = torch.tensor([est], device=dev, dtype=torch.float64)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                est = float(tt.item())
            for _ in range(max(0, min(4000, int(args.prewarm_ms * 1e-3 / max(est, 1e-5)) - 4))):
                step()
            torch.cuda.synchronize()
            if trainer is not None:      # a training step MOVES the scene: the timed steps start from the D2 scene again
                with torch.no_grad():
                    for p_, p0_ in zip(model.parameters(), train_snapshot):
                        p_.copy_(p0_)
                    for n_ in trainer.optimizer.names:
                        trainer.optimizer.exp_avg[n_].zero_()
                        trainer.optimizer.exp_avg_sq[n_].zero_()
                        trainer.optimizer.steps[n_] = 0
                torch.cuda.synchronize()
        for _ in range(args.warmup):
            step()
        barrier()
        t0_ = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        mine = time.perf_counter() - t0_
        if world > 1:
            tt = torch.tensor([mine], device=dev, dtype=torch.float64)
            every = [torch.zeros_like(tt) for _ in range(world)]
            dist.all_gather(every, tt)
            per_rank = [float(t_.item()) for t_ in every]
            return max(per_rank), per_rank
        return mine, [mine]

    coll_bytes = {}          # shard mode -> {collective: bytes this rank hands to it per step}

    def collective_ms_per_step(k_steps: int = 3):
        """Milliseconds per step this rank spends inside collectives (events around every exchange / all-reduce),
        measured in a few extra steps after the timed region -> (ms per step, collective calls per step)."""
        if world == 1 and not args.force_dist:
            return None, 0
        from tinysplat_amd._comm import collective_timer
        barrier()
        collective_timer.start()
        for _ in range(k_steps):
            step()
        torch.cuda.synchronize()
        by_label = collections.OrderedDict()
        for lab, nb in collective_timer.bytes:
            by_label[lab] = by_label.get(lab, 0) + nb
        coll_bytes[step_mode[0]] = {lab: nb // k_steps for lab, nb in by_label.items()}
        ms_, calls_ = collective_timer.stop()
        return ms_ / k_steps, calls_ // k_steps

    balanced = None
    if args.balance_stripes and gshard is not None and world > 1 and step_mode[0] == "gaussians":
        # real ranks: a few frames with equal rows, every rank hands in the work of its own tile rows, all ranks
        # derive the same balanced stripes and re-cut (outside the timed region)
        from tinysplat_amd import frame as _fr
        from tinysplat_amd.sharded import StripeBalancer, row_work
        bal = StripeBalancer(gshard[1])
        for _ in range(2):
            step()
            b_ = _fr.last_binning[dev.index]
            if b_.cam.wide_tiles:
                break
            gshard[1] = bal.update(row_work(b_.tile_bins, b_.cam.tile_bounds_x))
        balanced = list(gshard[1].stripes)
        if rank == 0:
            _log(f"work-balanced stripes (tile rows): {balanced}")
    elif args.balance_stripes and gshard is not None:
        balanced = list(gshard[1].stripes)
    if rank == 0:
        _log(f"timing {args.steps} steps ({step_mode[0] if world > 1 else 'single GPU'})")
    dt, dt_ranks = time_steps()
    if args.dump_outputs and rank == 0:
        # the parameters' gradients of the step's own model (--train-step: the parameters the step updated)
        src = gshard[0] if (gshard is not None and step_mode[0] == "gaussians") else model
        names = ("means", "colors_dc", "colors_rest", "scales", "quats", "opacities")
        arrays = dict(last_out)
        if trainer is not None:
            arrays.update({nm: getattr(src, nm) for nm in names})
        elif not args.forward_only:
            arrays.update({f"grad_{nm}": getattr(src, nm).grad for nm in names
                           if getattr(src, nm).grad is not None})
        dump_outputs(args.dump_outputs, arrays)
        _log(f"outputs of the last timed step written to {args.dump_outputs}: {', '.join(sorted(arrays))}")
    coll_ms, coll_calls = collective_ms_per_step() if args.full else (None, 0)
    second = None
    if both_modes:                      # the other design beside it, same scene, same K and W
        step_mode[0] = "replicated"
        if rank == 0:
            _log(f"timing {args.steps} steps (replicated parameters + one all-reduce)")
        dt2, dt2_ranks = time_steps()
        c2_ms, c2_calls = collective_ms_per_step()
        second = {"shard_mode": "replicated", "ms_per_step": dt2 / args.steps * 1e3,
                  "value": n * w * h / (dt2 / args.steps),
                  "rank_ms_min": min(dt2_ranks) / args.steps * 1e3, "rank_ms_max": max(dt2_ranks) / args.steps * 1e3,
                  "collective_ms_per_step": c2_ms, "collective_calls_per_step": c2_calls,
                  "collective_bytes_per_step": coll_bytes.get("replicated")}
        step_mode[0] = mode_first

    world_seen = dist.get_world_size() if (world > 1 or args.force_dist) else 1
    if args.gather_calibration and rank == 0:
        run_gather_calibration(dev)

    # the same step with D2's loss evaluated by torch kernels inside it, as rounds 1 - 4 timed it (a sub-record, so that
    # the series stays comparable: `value` is the step with the analytic upstream gradient)
    with_loss = None
    if (args.full and world == 1 and args.upstream == "grad" and not args.forward_only and not args.train_step
            and args.emulate_ranks <= 1 and not args.force_dist):
        args.upstream = "loss"
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        k_loss = max(5, min(args.steps, 50))
        for _ in range(k_loss):
            step()
        torch.cuda.synchronize()
        with_loss = {"ms_per_step": (time.perf_counter() - t1) / k_loss * 1e3, "steps": k_loss,
                     "note": "--upstream loss: torch's dot / fill / mul kernels of L = (rgb * w).sum() inside the step "
                             "(what rounds 1 - 4 reported)"}
        args.upstream = "grad"

    # second figure: the reference's whole adapter call renders RGB AND depth (rasterize.py:47-51); the headline
    # workload (D5) is RGB only, so the like-for-like frame is timed beside it
    rgbd = None
    if (args.full and world == 1 and not args.depth and not args.forward_only and not args.train_step
            and args.emulate_ranks <= 1 and not args.force_dist and not args.no_rgbd_figure):
        def step_rgbd():
            for p_ in model.parameters():
                p_.grad = None
            rgb, extras = adapter(cam, (w, h), sh)
            backprop([(rgb, w_rgb), (extras["depth"], w_d)])
        for _ in range(3):
            step_rgbd()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        k_rgbd = max(5, min(args.steps, 20))
        for _ in range(k_rgbd):
            step_rgbd()
        torch.cuda.synchronize()
        dt_rgbd = (time.perf_counter() - t1) / k_rgbd
        rgbd = {"workload": "the same scene through the adapter call with its depth output (rasterize.py:26-62): RGB + "
                            "depth composited in one 4-channel pass, both differentiated",
                "ms_per_step": dt_rgbd * 1e3, "value": n * w * h / dt_rgbd, "steps": k_rgbd}
        for _ in range(2):          # back to the headline workload's binning statistics
            step()

    # scene statistics + per-entry timing (after the timed region)
    if args.full:
        ops.kernel_timer.start()
        for _ in range(max(1, args.profile_steps)):
            step()
        per_entry = ops.kernel_timer.stop()
    from tinysplat_amd import frame as _frame
    binning = _frame.last_binning[dev.index] if dev.index in _frame.last_binning else ops._bin_cache.get(dev.index)[1]
    isects = int(binning.num_intersects)
    tiles = int(binning.num_tiles)
    bins = binning.tile_bins
    max_per_tile = int((bins[:, 1] - bins[:, 0]).max().item()) if tiles else 0
    isects_listed = int(bins[:, 1].max().item()) if tiles else 0    # after tight binning (<= isects)
    if world > 1:
        tt = torch.tensor([isects, isects_listed], device=dev, dtype=torch.int64)
        dist.all_reduce(tt)
        isects_total, listed_total = int(tt[0].item()), int(tt[1].item())
    else:
        isects_total, listed_total = isects, isects_listed

    if rank == 0:
        p = w * h
        k = (sh + 1) ** 2
        ch = 4 if (args.depth or args.forward_only or args.train_step) else 3
        ms = dt / args.steps * 1e3
        value = n * p / (dt / args.steps)
        _log(f"timed: {ms:.3f} ms/step")
        pmc = None
        if args.full:
            per_step = {e: v[1] * v[0] / max(1, args.profile_steps) for e, v in per_entry.items()}   # ms / step
            stage_ms = collections.defaultdict(float)
            stage_entries = collections.defaultdict(list)
            for e, t_ in per_step.items():
                st = STAGE_OF.get(e)
                if st is not None:
                    stage_ms[st] += t_
                    stage_entries[st].append(e)
            # dominant stage = the D5 stage with the largest time on this rank; its dominant kernel is
            # the entry inside it with the largest time
            dom_stage = max(stage_ms.items(), key=lambda kv: kv[1])[0]
            dom_ms = stage_ms[dom_stage]
            dom_entry = max(stage_entries[dom_stage], key=lambda e: per_step[e])
            p_local = p if (world == 1 and args.emulate_ranks <= 1) else binning.cam.tile_rows * 16 * w
            # D5 priced with the pairs a launch actually processes (the tight lists); the figure with gsplat's
            # bounding-box pair count - pairs that are never scattered, sorted or composited - is kept beside it
            n_local = int(binning.n)              # Gaussians (or imported records) this rank's stages run over
            a_bytes = stage_alg_bytes(dom_stage, n_local, isects_listed, p_local, tiles, k, ch)
            a_bytes_bbox = stage_alg_bytes(dom_stage, n_local, isects, p_local, tiles, k, ch)
            full_tiles = (w + 15) // 16 * ((h + 15) // 16)
            frame_bytes = frame_alg_bytes(n, isects_total, p, full_tiles, k, args.depth)
            frame_bytes_listed = frame_alg_bytes(n, listed_total, p, full_tiles, k, args.depth)

            pmc, pmc_src = None, None
            if world == 1 and not args.no_pmc and not args.train_step:
                wl = ["--n", str(n), "--sh-degree", str(sh), "--width", str(w), "--height", str(h),
                      "--scale-mult", str(args.scale_mult)] + (["--depth"] if args.depth else []) \
                     + (["--spatial-sort"] if args.spatial_sort else []) \
                     + (["--forward-only"] if args.forward_only else []) \
                     + (["--emulate-ranks", str(args.emulate_ranks), "--emulate-rank", str(args.emulate_rank),
                         "--shard-mode", args.shard_mode] if args.emulate_ranks > 1 else [])
                _log("PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / SQ_INSTS_VALU)")
                pmc = collect_pmc(wl)
                _log("PMC passes done" if pmc else "PMC passes unavailable")
                pmc_src = "rocprofv3 --pmc passes of this run" if pmc else None
            if pmc is None and not args.no_pmc:          # (the PMC passes' own child runs pass --no-pmc: no counters there)
                tf = ROOT / "profiles" / "pmc_latest.json"
                if tf.exists() and (n, sh, w, h, args.depth) == (1_000_000, 3, 1920, 1080, False):
                    try:
                        pmc = json.loads(tf.read_text())
                        if not (isinstance(pmc, dict) and all(isinstance(v, dict) for v in pmc.values())):
                            raise ValueError("not a pmc_per_dispatch record")
                        pmc_src = "profiles/pmc_latest.json (committed; not collected in this run)"
                    except Exception:
                        pmc = None

            # FETCH_SIZE correction.  Wide coalesced reads: x2 (gfx950 tallies 128-B requests as 64 B,
            # MI355X_MICROARCH.md HBM section).  Gathers of 48-byte records are not covered by that calibration, so
            # the PMC passes also run ts_bench_gather48 on a known count: a 16-byte-aligned 48-byte record lies in
            # 1.25 128-byte lines on average (160 B fetched per record when every gather misses the L2s).  The raw
            # FETCH_SIZE per record decides the factor applied to the gather-dominated kernels: ~80 B -> the same
            # half-tally (x2), ~160 B -> x1.
            GATHER_ENTRIES = ("ts_raster_fwd", "ts_raster_bwd", "ts_reduce_partials")
            cal = (pmc or {}).get("gather48_calibration")
            gather_factor, gather_raw = 2.0, None
            if cal and "fetch_kib" in cal:
                gather_raw = cal["fetch_kib"] * 1024.0 / GATHER_CAL_GATHERS
                gather_factor = 2.0 if gather_raw < 120.0 else 1.0

            def traffic_of(entries):
                """HBM bytes per step of the entries: (factor x FETCH_SIZE + WRITE_SIZE) KiB."""
                if not pmc:
                    return None
                tot = 0.0
                for e in entries:
                    c = pmc.get(e)
                    if not c or "fetch_kib" not in c or "write_kib" not in c:
                        return None
                    launches = per_entry[e][0] / max(1, args.profile_steps)
                    f_ = gather_factor if e in GATHER_ENTRIES else 2.0
                    tot += (f_ * c["fetch_kib"] + c["write_kib"]) * 1024.0 * launches
                return tot

            bw_meas = None if args.no_bandwidth else measure_read_bandwidth(dev)

            # ---- roofline of the DOMINANT KERNEL, SURVEY 8(d).  Numerator and denominator cover the SAME scope (ADVICE
            # r4): the bytes that kernel itself moves - its share of the D5 stage - priced on the pairs the launch really
            # lists, over that kernel's own launch duration (HIP events on the stream it runs on), against the 8 TB/s HBM
            # peak.  Sub-records: the whole D5 stage (all its entries: stage bytes over stage time) and the same two
            # figures priced on gsplat's bounding-box pair count I = sum of num_tiles_hit - pairs this build never
            # scatters, sorts or composites included -, labelled as such.
            dom_kernel_ms = per_step[dom_entry]
            k_bytes = entry_alg_bytes(dom_entry, dom_stage, n_local, isects_listed, p_local, tiles, k, ch)
            k_bytes_bbox = entry_alg_bytes(dom_entry, dom_stage, n_local, isects, p_local, tiles, k, ch)
            kernel_scope = k_bytes is not None
            if not kernel_scope:                  # a stage whose entries are not priced one by one: the stage is the scope
                k_bytes, k_bytes_bbox, scope_ms = a_bytes, a_bytes_bbox, dom_ms
            else:
                scope_ms = dom_kernel_ms
            # FROZEN DEFINITION (round 6, VERDICT r5 item 8 - do not redefine): roofline.frac = SURVEY 8(d) D5's bytes of the
            # dominant kernel's OWN share, priced LITERALLY - on gsplat's pair count I = sum of num_tiles_hit -, over that
            # kernel's own launch duration, against the 8 TB/s HBM peak.  It is what a reader recomputes from D5, I, P, N and
            # the kernel's time (the review's 0.136 of round 5; the line's own frac read 0.87 / 0.135 / 0.0995 in rounds
            # 3 / 4 / 5 under three different definitions).  Everything else is a NAMED sub-record: `listed_pairs` (the same
            # formula on the pairs this build's tight lists really hold), `stage` (all entries of the D5 stage: stage
            # bytes over stage time, both pair counts), `valu` (the vector-ALU view of the same kernel).
            achieved_literal = k_bytes_bbox / (scope_ms * 1e-3) / 1e9
            achieved_listed = k_bytes / (scope_ms * 1e-3) / 1e9
            achieved_stage = a_bytes / (dom_ms * 1e-3) / 1e9
            achieved_stage_literal = a_bytes_bbox / (dom_ms * 1e-3) / 1e9
            roofline = {
                "bound": "hbm", "kernel": dom_entry, "stage": dom_stage, "kernel_ms": dom_kernel_ms,
                "definition": "D5-literal bytes of the dominant kernel's own share (gsplat's pair count I = sum of "
                              "num_tiles_hit) / that kernel's own launch duration / 8 TB/s; frozen in round 6",
                "scope": "the kernel's own bytes over the kernel's own time" if kernel_scope else
                         "the D5 stage's bytes over the time of all its entries",
                "alg_bytes": k_bytes_bbox, "pairs": isects,
                "achieved": achieved_literal, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved_literal / HBM_PEAK_GBS,
                "traffic": traffic_of([dom_entry] if kernel_scope else stage_entries[dom_stage]), "traffic_source": pmc_src,
                "peak_read_measured": bw_meas,
                "frac_of_measured": None if bw_meas is None else achieved_literal / bw_meas,
                "listed_pairs": {"pairs": isects_listed,
                                 "note": "the same formula priced on the pairs the launch really lists (tight lists: only "
                                         "the tiles the alpha >= 1/255 level set can reach) - round 5's top-level figure",
                                 "alg_bytes": k_bytes, "achieved": achieved_listed, "frac": achieved_listed / HBM_PEAK_GBS},
                "stage": {"entries": sorted(stage_entries[dom_stage]), "ms": dom_ms,
                          "alg_bytes": a_bytes_bbox, "achieved": achieved_stage_literal,
                          "frac": achieved_stage_literal / HBM_PEAK_GBS,
                          "listed_pairs": {"alg_bytes": a_bytes, "achieved": achieved_stage,
                                           "frac": achieved_stage / HBM_PEAK_GBS},
                          "traffic": traffic_of(stage_entries[dom_stage]),
                          "stage_bytes_over_kernel_time_frac": a_bytes_bbox / (dom_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "stage_bytes_over_kernel_time_note": "round 4's top-level figure (numerator: two entries, "
                                                               "denominator: one) - kept for comparison only"},
                "fetch_correction": {"streaming": 2.0, "gather_kernels": gather_factor,
                                     "gather48_raw_fetch_bytes_per_record": gather_raw,
                                     "gather48_expected_bytes_per_record": 160.0,
                                     "gather_kernels_list": list(GATHER_ENTRIES)},
            }
            frame_gbs = frame_bytes / (ms * 1e-3) / 1e9
            frame_gbs_listed = frame_bytes_listed / (ms * 1e-3) / 1e9
            # whole frame: D5's frame bytes priced on the listed pairs over the timed step; gsplat's pair count beside it
            frame_roofline = {"definition": "D5's frame bytes, priced literally (gsplat's pair count), over the timed step",
                              "alg_bytes": frame_bytes, "pairs": isects_total, "achieved": frame_gbs,
                              "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": frame_gbs / HBM_PEAK_GBS,
                              "listed_pairs": {"pairs": listed_total, "alg_bytes": frame_bytes_listed,
                                               "achieved": frame_gbs_listed, "frac": frame_gbs_listed / HBM_PEAK_GBS},
                              "peak_read_measured": bw_meas,
                              "frac_of_measured": None if bw_meas is None else frame_gbs / bw_meas}
            # the compositing kernels against the vector ALUs (D4's second figure)
            valu = {}
            for e in ("ts_raster_fwd", "ts_raster_bwd"):
                if e not in per_step:
                    continue
                t_s = per_step[e] * 1e-3
                ent = {"kernel_ms": per_step[e],
                       # D4: 256 pixel x Gaussian evaluations per listed pair (upper bound, before early-out)
                       "pair_evals_per_s": 256.0 * isects_listed / t_s,
                       "pair_evals_per_s_gsplat_lists": 256.0 * isects / t_s}
                c = (pmc or {}).get(e)
                if c and "valu_insts" in c:
                    lane_ops = c["valu_insts"] * 64.0
                    ent.update({"valu_wave_insts": c["valu_insts"],
                                "valu_insts_per_listed_pair": c["valu_insts"] / max(1, isects_listed),
                                "lane_ops_per_s": lane_ops / t_s, "peak_lane_ops_per_s": VALU_LANE_OPS_PEAK,
                                "peak_note": "256 CUs x 4 SIMD-32 x 2.4 GHz: a wave64 instruction per 2 cycles per SIMD",
                                "frac": lane_ops / t_s / VALU_LANE_OPS_PEAK,
                                # counting every VALU instruction as one FMA (2 flops): an upper bound
                                "tflops_if_all_fma": 2.0 * lane_ops / t_s / 1e12,
                                "peak_tflops_fp32_vector": VALU_FP32_PEAK_TFLOPS})
                    if "valu_active_quads" in c and "sq_busy_cycles" in c:
                        cycles = c["sq_busy_cycles"] / SQ_INSTANCES          # shader cycles of one launch (under the profiler)
                        ent.update({"kernel_cycles": cycles,
                                    # SQ_ACTIVE_INST_VALU counts quad-cycles a wave's VALU instruction is in flight: a
                                    # wave-side time (>= 1 quad per instruction), so the ratio can exceed 1 with several
                                    # waves per SIMD; kept as VERDICT r3 defined it
                                    "valu_busy": c["valu_active_quads"] * 4.0 / (SIMDS * cycles),
                                    "cycles_per_valu_inst": c["valu_active_quads"] * 4.0 / c["valu_wave_insts"]
                                    if "valu_wave_insts" in c else c["valu_active_quads"] * 4.0 / c["valu_insts"],
                                    "simd_cycles_per_valu_inst": SIMDS * cycles / c["valu_insts"],
                                    "resident_waves_per_simd": c.get("wave_quads", 0.0) * 4.0 / (SIMDS * cycles)})
                if "frac" in ent:
                    # the same instructions charged what their CLASSES cost on the pipe instead of 2 cycles each (round 4's
                    # micro-benchmarks: v_cmp 4, v_exp / v_rcp 6.2, DPP / select ~3, lane swaps 6.5): the hot loops' ISA priced
                    # that way averages 2.71 (forward) / 2.55 (backward) cycles per instruction - a
                    # STATIC weight from the listing, applied to the counted instructions
                    wgt = CLASS_WEIGHT.get(e)
                    if wgt:
                        ent["class_weighted"] = {"avg_pipe_cycles_per_inst": wgt, "frac": ent["frac"] * wgt / 2.0,
                                                 "note": "valu.frac with every instruction at its class's pipe cost (static "
                                                         "weight from the priced ISA of the hot loops, DESIGN.md section 4)"}
                valu[e] = ent
            roofline["valu"] = valu.get(dom_entry)
        out = {
            "metric": "Gaussians*pixels/s forward only (no_grad, RGB+depth)" if args.forward_only else
                      "Gaussians*pixels/s fwd+bwd" if not args.train_step else
                      "Gaussians*pixels/s of a full training step (render RGB+depth, loss, backward, Adam)",
            "value": value, "unit": "Gaussians*pixels/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "prewarm_ms": args.prewarm_ms, "ms_per_step": ms, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{n} random Gaussians, SH degree {sh}, {w}x{h}, fwd+bwd "
                                   f"({'RGB+depth' if args.depth else 'RGB'}), BASELINE configs[2]"
                                   if (n, sh, w, h) == (1_000_000, 3, 1920, 1080) else
                                   f"{n} random Gaussians, SH degree {sh}, {w}x{h}, fwd+bwd "
                                   f"({'RGB+depth' if args.depth else 'RGB'})",
                       "intersections": isects_total, "intersections_listed": listed_total,
                       "max_per_tile": max_per_tile,
                       "parallelism": ((f"Gaussian shards + tile-row stripes x{world} (records / gradient rows by all_to_all)"
                                        if (gshard is not None and mode_first == "gaussians") else
                                        f"tile-row stripes x{world}, replicated parameters, one all-reduce")
                                       + (" (ALL RANKS ON ONE GPU: functional test, not a measurement)"
                                          if args.single_device else "")) if world > 1 else "single GPU",
                       "scale_mult": args.scale_mult,
                       "upstream": ("v_out = w handed to autograd.backward (the analytic dL/d image of D2's "
                                    "L = (rgb * w).sum()): no loss kernels inside the step" if args.upstream == "grad"
                                    else "D2's loss evaluated by torch kernels inside the step (rounds 1-4)"),
                       "host_cpus": (f"cores of the GPU's NUMA node ({host_cpus})" if host_cpus else "not pinned"),
                       "tile_lists": {0: "16x16 (gsplat's)", 1: "32x16 lists, 32x16 waves",
                                      2: "32x16 lists (pairs of 16x16 tiles), one wave per 16x16 tile"}.get(
                                          _frame._list_mode(dev.index, tiles), "?")
                                      + (" (auto)" if _frame.WIDE_TILES == "auto" else ""),
                       "gaussian_order": "Morton curve of the means (--spatial-sort)" if args.spatial_sort
                                         else "as generated (i.i.d.)",
                       **({"stripes": balanced, "stripes_policy": "balanced by the lists' work"} if balanced else {}),
                       **({"top_third": args.top_third} if args.top_third else {}),
                       **({"emulated_stripe": f"{args.emulate_rank} of {args.emulate_ranks} on ONE GPU "
                                              "(per-rank estimate, not a multi-GPU measurement), shard mode "
                                              + args.shard_mode}
                          if args.emulate_ranks > 1 and world == 1 else {})},
        }
        if args.full:
            out.update({
                "roofline": roofline,
                "frame_roofline": frame_roofline,
                "valu_roofline": valu,
                "stages_ms": {k_: round(v, 4) for k_, v in sorted(stage_ms.items())},
                "entries_ms": {k_: round(v, 4) for k_, v in sorted(per_step.items())},
            })
            if args.train_step:
                # what the optimiser part of the step costs against what it must move.  Fused (default): the
                # parameter-stage backward kernels update p, m, v in place from the gradient in registers - per Gaussian the
                # 2-D gradients in (52 B + 4 B radii + 12 B means for the view directions) and p, m, v of all 14 + 3 K
                # parameters read and written (24 B each); the two-launch form writes and re-reads the gradients on top.
                npar = 14 + 3 * k
                fused = "ts_project_bwd_adam" in per_step
                ents = [e for e in ("ts_sh_colors_bwd_adam", "ts_project_bwd_adam", "ts_sh_colors_bwd", "ts_project_bwd",
                                    "ts_adam_step") if e in per_step]
                t_ms = sum(per_step[e] for e in ents)
                b_alg = n * (68.0 + 24.0 * npar + (0.0 if fused else 8.0 * npar))
                out["train_step_roofline"] = {
                    "fused_adam": fused, "entries": {e: round(per_step[e], 4) for e in ents}, "ms": t_ms,
                    "alg_bytes": b_alg, "achieved": b_alg / (t_ms * 1e-3) / 1e9 if t_ms > 0 else None, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": (b_alg / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if t_ms > 0 else None,
                    "photometric_loss_ms": per_step.get("ts_photometric_loss_rgbd", per_step.get("ts_photometric_loss_planes")),
                    "note": "parameter-stage backward + Adam of the training step: algorithmic bytes (p, m, v read and written, "
                            "the 2-D gradients read" + ("" if fused else ", the six gradient tensors written and read") +
                            ") over the time of the entries listed"}
        if world > 1 or args.force_dist:
            # what ran, said by the line itself: the design, whether the preflight sent the ranks to the other one,
            # how many ranks the backend saw, the spread over the ranks and the time inside collectives
            out["multi_gpu"] = {
                "shard_mode": mode_first, "shard_mode_requested": shard_info["requested"],
                "shard_mode_fallback": shard_info["fallback"], "preflight": shard_info["preflight"],
                "backend": args.backend, "rccl_ranks": world_seen if args.backend == "nccl" else None,
                "ranks": world_seen,
                "rank_ms_min": min(dt_ranks) / args.steps * 1e3, "rank_ms_max": max(dt_ranks) / args.steps * 1e3,
                "collective_ms_per_step": coll_ms, "collective_calls_per_step": coll_calls,
                "collective_bytes_per_step": coll_bytes.get(mode_first),
                "collective_bytes_note": "rank 0's send buffer per collective and step (an all-reduce: the reduced buffer)",
                "collective_ms_note": "rank 0, events around every all_to_all / all-reduce, in 3 extra steps after the "
                                      "timed region (gloo: host-side calls, not timed)"}
            if second is not None:
                out["multi_gpu"]["replicated_mode"] = second
        if rgbd is not None:
            out["frame_rgbd"] = rgbd
        if with_loss is not None:
            out["with_loss_kernels"] = with_loss
        if pmc:
            out["pmc_per_dispatch"] = {e: {k_: round(v, 1) for k_, v in c.items()} for e, c in sorted(pmc.items())}
        if args.full and world == 1 and not args.no_cpu_baseline:
            _log("CPU baseline (oracle on the host cores)")
            out["cpu_baseline"] = cpu_baseline_guarded()
            _log("CPU baseline done")
    if world > 1 or args.force_dist:
        dist.destroy_process_group()
    if rank == 0:
        # RCCL prints its version banner through C stdio, which is flushed at exit: push it out now
        # so that the JSON line is the last line of output
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
