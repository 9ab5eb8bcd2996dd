#!/usr/bin/env python
"""Times the iso-surface mesh extraction (tinysplat_amd.mesh) with device events after a warm-up; prints one JSON line
per measurement (ms).

  * ``extract_mesh``: the whole call on N Gaussians at one resolution, with the vertex and face counts, the active
    brick share, the chunks and the peak memory over the model against the workspace cap;
  * its parts, per entry of the C ABI (``ops.kernel_timer``: events around every launch); what remains of the whole is
    torch (nonzero, scans, ``unique``) and host time;
  * ``fallback share``: the corner queries that took ``ts_knn``'s brute-force pass, from a separate run that asks every
    chunk's search for its statistics;
  * ``--dense``: the same call with ``sparse=False`` (every brick), the baseline of the sparse grid;
  * ``--colors``: the call with ``colors=True`` at ``--color-degree`` (seeded coefficients of 16 bands): the colour
    stage (``ts_field_colors``) is listed beside the normals stage of the same run, with the bytes it must move
    (``V x 16 x (40 + 12 (degree + 1)^2) + 12 V``, an upper bound before cache reuse) as a share of the HBM peak;
  * ``--target-faces N``: the call with ``target_faces=N`` (section 6i); the simplification is then also timed alone on
    the unsimplified mesh (``simplify_mesh`` without a model), with its entries' times, the resolution ``r`` the budget
    search chose, its probes, the clusters, the faces in and out and the stage's peak memory against the cap;
  * ``--clean``: the call with ``clean=CleanConfig(keep_largest=1)`` (section 6j: the edge step and the components); the
    clean-up is then also timed alone on the mesh it meets in that call (simplified with ``--target-faces``, without
    attributes), with its entries' times, torch's three sorts timed on the same keys, what it removed and its peak memory
    over the input mesh; and ``mesh_components`` alone on the unsimplified mesh, the union-find at the largest size.

    python tools/time_mesh.py [--scene sheet|volume] [--n 1000000] [--resolution 256] [--dense] [--colors]
                              [--color-degree 3] [--target-faces N] [--clean] [--reps 3] [--out f.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from tinysplat_amd import _lib  # noqa: E402
from tinysplat_amd.extract import EXTRACT_K, pack_model  # noqa: E402
from tinysplat_amd.mesh import BRICK_CORNERS, MeshConfig, extract_mesh  # noqa: E402
from tinysplat_amd.ops import _ptr, _stream, kernel_timer  # noqa: E402
from tinysplat_amd.synthetic import make_scene  # noqa: E402
from time_extract import sheet_scene, timed  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12               # bytes / s, the MI355X's HBM3E


@torch.no_grad()
def fallback_share(model, pk, cfg, active, grid, chunk_bricks=1024):
    """The share of the active bricks' corner queries that take ``ts_knn``'s brute-force pass."""
    lib = _lib.load()
    dev = torch.device(DEV)
    n = pk.means.shape[0]
    q = chunk_bricks * BRICK_CORNERS
    ws = torch.empty(int(lib.ts_knn_ws_bytes(n, q, EXTRACT_K)), dtype=torch.uint8, device=dev)
    corners = torch.empty((q, 3), device=dev)
    dist = torch.empty((q, EXTRACT_K), device=dev)
    idx = torch.empty((q, EXTRACT_K), dtype=torch.int32, device=dev)
    stats = torch.zeros((2,), dtype=torch.int32, device=dev)
    took = 0
    s = _stream(dev)
    for b0 in range(0, active.shape[0], chunk_bricks):
        ids = active[b0:b0 + chunk_bricks]
        b = int(ids.shape[0])
        assert lib.ts_mesh_corners(b, _ptr(ids), grid.grid_host, grid.cells_host, _ptr(corners), s) == 0
        assert lib.ts_knn(n, _ptr(pk.means), b * BRICK_CORNERS, _ptr(corners), EXTRACT_K, _ptr(dist), _ptr(idx),
                          _ptr(ws), _ptr(stats), s) == 0
        took += int(stats[0])
    return took / max(1, active.shape[0] * BRICK_CORNERS)


@torch.no_grad()
def clean_stage(model, pk, cfg, ccfg, reps, emit, shape):
    """The clean-up alone on the mesh ``extract_mesh`` hands it, and the components of the unsimplified mesh."""
    import dataclasses
    from tinysplat_amd.clean import clean_mesh, mesh_components
    bare = dataclasses.replace(cfg, normals=False, colors=False, clean=None)
    met = extract_mesh(model, bare, packed=pk)
    v, f = int(met.vertices.shape[0]), int(met.faces.shape[0])
    input_bytes = met.vertices.numel() * 4 + met.faces.numel() * 4

    def stage():
        return clean_mesh(met, ccfg)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stage_ms = timed(stage, reps)
    peak = torch.cuda.max_memory_allocated() - base
    kernel_timer.start()
    stage()
    parts = kernel_timer.stop()
    kernels = {name: round(launches * mean_ms, 4) for name, (launches, mean_ms) in sorted(parts.items())}
    out, info = clean_mesh(met, ccfg, return_debug=True)
    # torch's sorts of the edge step, on the same keys: the keys alone, the weights, the keys again (stable)
    lib = _lib.load()
    keys = torch.empty((3 * f,), dtype=torch.int64, device=DEV)
    weights = torch.empty((f,), dtype=torch.float64, device=DEV)
    s = _stream(torch.device(DEV))
    assert lib.ts_clean_edge_keys(v, f, _ptr(met.faces), _ptr(keys), s) == 0
    assert lib.ts_clean_face_weights(v, f, _ptr(met.vertices), _ptr(met.faces), _ptr(weights), s) == 0
    sorts = {"keys alone": round(timed(lambda: torch.sort(keys), reps), 4),
             "weights, stable": round(timed(lambda: torch.sort(weights, descending=True, stable=True), reps), 4),
             "keys, stable": round(timed(lambda: torch.sort(keys, stable=True), reps), 4)}
    del keys, weights
    inside = sum(kernels.values()) + sum(sorts.values())
    emit("clean stage", stage_ms, faces_in=f, faces_out=int(out.faces.shape[0]), vertices_in=v,
         vertices_out=int(out.vertices.shape[0]), nonmanifold_edges=info["nonmanifold_edges"],
         removed_nonmanifold_faces=info["removed_nonmanifold_faces"], components=int(info["sizes"].shape[0]),
         kept_components=int(info["kept_components"].shape[0]), kernels_ms=kernels, torch_sorts_ms=sorts,
         other_torch_and_host_ms=round(stage_ms - inside, 4), peak_mib=round(peak / 2 ** 20, 1),
         input_mesh_mib=round(input_bytes / 2 ** 20, 1), **shape)
    del met, out
    plain = extract_mesh(model, dataclasses.replace(bare, target_faces=None), packed=pk)

    def comps():
        return mesh_components(plain)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    comps_ms = timed(comps, reps)
    peak = torch.cuda.max_memory_allocated() - base
    kernel_timer.start()
    sizes = comps()[3]
    parts = kernel_timer.stop()
    launches, mean_ms = parts["ts_clean_components"]
    emit("components, unsimplified", comps_ms, faces=int(plain.faces.shape[0]), vertices=int(plain.vertices.shape[0]),
         components=int(sizes.shape[0]), largest=int(sizes.max()) if sizes.shape[0] else 0,
         ts_clean_components_ms=round(launches * mean_ms, 4), peak_mib=round(peak / 2 ** 20, 1), **shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--scene", choices=("volume", "sheet"), default="sheet")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--colors", action="store_true")
    ap.add_argument("--color-degree", type=int, default=3)
    ap.add_argument("--target-faces", type=int, default=None)
    ap.add_argument("--clean", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
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
    if args.colors:
        g = torch.Generator(device=DEV).manual_seed(1)
        model.colors_rest = 0.3 * torch.randn((args.n, 15, 3), generator=g, device=DEV)
        model.active_sh_degree = 3
    pk = pack_model(model)
    from tinysplat_amd.clean import CleanConfig
    ccfg = CleanConfig(keep_largest=1) if args.clean else None
    cfg = MeshConfig(resolution=args.resolution, sparse=not args.dense, colors=args.colors,
                     color_sh_degree=args.color_degree if args.colors else None, target_faces=args.target_faces,
                     clean=ccfg)
    shape = dict(scene=args.scene, n=args.n, resolution=args.resolution, sparse=cfg.sparse)
    if args.colors:
        shape["color_degree"] = args.color_degree
    if args.target_faces is not None:
        shape["target_faces"] = args.target_faces
    if args.clean:
        shape["clean"] = "keep_largest=1"

    def run():
        return extract_mesh(model, cfg, packed=pk)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    total = timed(run, args.reps)
    peak = torch.cuda.max_memory_allocated() - base
    mesh = run()
    # the bricks, from a run of the marking stage alone
    from tinysplat_amd._bricks import BrickGrid
    from tinysplat_amd.mesh import gaussian_boxes
    boxes = gaussian_boxes(model, cfg.extent_sigmas)
    grid = BrickGrid(boxes[:, :3].amin(0).tolist(), boxes[:, 3:].amax(0).tolist(), cfg.resolution,
                     cfg.max_workspace_bytes)
    cells, bricks = grid.cells, grid.total_bricks
    lib = _lib.load()

    def mark(flags):
        assert lib.ts_mesh_mark(args.n, _ptr(boxes), grid.grid_host, grid.cells_host, _ptr(flags),
                                _stream(torch.device(DEV))) == 0
    marked = grid.active_bricks(True, mark, DEV)
    active = marked if cfg.sparse else grid.active_bricks(False, None, DEV)
    emit("extract_mesh", total, vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]), cells=cells,
         bricks=bricks, marked_bricks=int(marked.shape[0]), evaluated_bricks=int(active.shape[0]),
         active_share=round(int(marked.shape[0]) / bricks, 5), peak_mib=round(peak / 2 ** 20, 1),
         cap_mib=cfg.max_workspace_bytes >> 20, **shape)
    kernel_timer.start()
    run()
    parts = kernel_timer.stop()
    inside = 0.0
    for name, (launches, mean_ms) in sorted(parts.items()):
        inside += launches * mean_ms
        emit("part " + name, launches * mean_ms, launches=launches, **shape)
    emit("part torch and host (the rest)", total - inside, **shape)
    if args.colors:
        v = int(mesh.vertices.shape[0])
        launches, mean_ms = parts["ts_field_colors"]
        ms = launches * mean_ms
        nbytes = v * EXTRACT_K * (40 + 12 * (args.color_degree + 1) ** 2) + 12 * v
        n_launches, n_mean = parts["ts_extract_normals"]
        emit("colour stage", ms, vertices=v, bytes_upper_bound=nbytes, gbytes_per_s=round(nbytes / ms / 1e6, 1),
             share_of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 4), normals_stage_ms=round(n_launches * n_mean, 4),
             **shape)
    if args.target_faces is not None:
        import dataclasses
        from tinysplat_amd.simplify import SimplifyConfig, simplify_mesh
        plain = extract_mesh(model, dataclasses.replace(cfg, target_faces=None, normals=False, colors=False, clean=None),
                             packed=pk)
        scfg = SimplifyConfig(target_faces=args.target_faces, max_workspace_bytes=cfg.max_workspace_bytes)

        def stage():
            return simplify_mesh(plain, scfg)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        stage_ms = timed(stage, args.reps)
        stage_peak = torch.cuda.max_memory_allocated() - base
        kernel_timer.start()
        out, info = simplify_mesh(plain, scfg, return_debug=True)
        stage_parts = kernel_timer.stop()
        kernels = {name: round(launches * mean_ms, 4) for name, (launches, mean_ms) in sorted(stage_parts.items())}
        emit("simplify stage", stage_ms, faces_in=int(plain.faces.shape[0]), faces_out=int(out.faces.shape[0]),
             vertices_in=int(plain.vertices.shape[0]), vertices_out=int(out.vertices.shape[0]), r=info["r"],
             cell_size=info["cell_size"], probes=info["probes"], clusters=info.get("clusters"),
             pieces=info.get("pieces"), kernels_ms=kernels,
             torch_and_host_ms=round(stage_ms - sum(kernels.values()), 4), peak_mib=round(stage_peak / 2 ** 20, 1),
             cap_mib=cfg.max_workspace_bytes >> 20, **shape)
        del plain, out
    if args.clean:
        clean_stage(model, pk, cfg, ccfg, args.reps, emit, shape)
    emit("fallback share", 0.0, share=round(fallback_share(model, pk, cfg, active, grid), 5),
         corner_queries=int(active.shape[0]) * BRICK_CORNERS, **shape)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
