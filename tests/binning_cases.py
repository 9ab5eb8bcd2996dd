"""Scaffolding shared by the tests of the tile-list builders (csrc/binning.hip): the projected inputs of a scene, the
list-building stages of one FORM driven through the C ABI, and the bit-for-bit comparison of two such runs.

n = 2^18 + 77 sits just above the two-hop threshold (193 chunks of 1359 Gaussians, a ragged last one); 400 x 304 is
25 x 19 = 475 tiles, i.e. 14 full groups of 32 lists and one of 27."""
import ctypes

import torch

from tinysplat_amd import _lib, ops
from tinysplat_amd.rasterizer import project_args, tile_bounds
from tinysplat_amd.synthetic import make_scene

DEV = "cuda:0"
N = (1 << 18) + 77
W, H = 400, 304
SENTINEL = -1
UNSET = -7
MATRIX, GROUP, WALK = "matrix", "group", "one walk"
_scenes = {}


def chunks(n):
    """bin_num_chunks of csrc/binning.hip -> (chunks, Gaussians per chunk)"""
    per = min(max(n // 192, 1024), 4096)
    b = min(max((n + per - 1) // per, 1), 512)
    return b, (n + b - 1) // b


def projected(clustered=0.0, tile_rows=None, enlarge=None, dims=(W, H)):
    """2-D inputs of the binning stages (projection, scan, packed records for the tight lists), once per scene.
    enlarge = (share, factor): the first `share` of the Gaussians get `factor` times the extent"""
    key = (clustered, tile_rows, enlarge, dims)
    if key not in _scenes:
        lib = _lib.load()
        dev = torch.device(DEV)
        w, h = dims
        model, cam = make_scene(N, 0, w, h, seed=41, clustered=clustered)
        if enlarge:
            with torch.no_grad():
                model.scales[:int(N * enlarge[0])] += torch.log(torch.tensor(float(enlarge[1])))
        md = model.to(dev)
        with torch.no_grad():
            xys, depths, radii, conics, nth, _ = ops.project_gaussians(*project_args(md, cam, (w, h), DEV),
                                                                       tile_rows=tile_rows)
            opac = torch.sigmoid(md.opacities).reshape(-1).contiguous()
        colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(2)).to(dev)
        s, p = ops._stream(dev), ops._ptr
        cum = torch.empty((N,), dtype=torch.int32, device=dev)
        ws = torch.empty((int(lib.ts_scan_ws_ints(N)),), dtype=torch.int32, device=dev)
        ops._call("ts_scan_tiles", lib.ts_scan_tiles, N, p(nth), p(cum), p(ws), None, s)
        splats = torch.zeros((N, 12), dtype=torch.float32, device=dev)
        cam16 = ops._camera(0.0, 0.0, 0.0, 0.0, h, w, tile_bounds((w, h)), tile_rows=tile_rows)
        ops._call("ts_pack_splats", lib.ts_pack_splats, N, 3, 0, p(xys), p(radii), p(conics), p(colors), p(opac), p(cum),
                  cam16, None, p(splats), s)
        torch.cuda.synchronize()
        _scenes[key] = dict(n=N, xys=xys, depths=depths, radii=radii, cum=cum, splats=splats, total=int(cum[-1]),
                            tile_rows=tile_rows, dims=dims)
    return _scenes[key]


def chain(inp, form, wide=False, hints=0, capacity=-1):
    """the list-building stages in one form (MATRIX with the scratch buffer given, GROUP or WALK) -> everything a later
    stage or the host reads.  inp["splats"] may be None: bounding-box lists"""
    lib = _lib.load()
    dev = torch.device(DEV)
    n, total = inp["n"], inp["total"]
    w, h = inp["dims"]
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, h, w, tile_bounds((w, h)), tile_rows=inp["tile_rows"], wide_tiles=wide)
    cam.hints = hints
    nt = int(lib.ts_num_tiles(ctypes.byref(cam)))
    i32 = dict(dtype=torch.int32, device=dev)
    s, p = ops._stream(dev), ops._ptr
    xys, rad, tl, depths, cum = inp["xys"], inp["radii"], p(inp["splats"]), inp["depths"], inp["cum"]
    bin_ws = torch.full((int(lib.ts_bin_ws_ints(n, nt)),), UNSET, **i32)
    tile_bins = torch.full((nt, 2), UNSET, **i32)
    bucket_ids = torch.full((total,), SENTINEL, **i32)
    ids = torch.full((total,), SENTINEL, **i32)
    longest = torch.full((1,), UNSET, **i32)
    spare = bin_ws.data_ptr() + 4 * (bin_ws.numel() - 1)
    matrix = None
    if form == WALK:
        assert lib.ts_bin_one_walk_form(n, nt) == 1
        ops._call("ts_bin_emit_groups", lib.ts_bin_emit_groups, n, p(xys), p(rad), tl, cam, p(cum), capacity, p(bin_ws),
                  p(ids), s)
        ops._call("ts_emit_offsets", lib.ts_emit_offsets, n, nt, p(bin_ws), p(tile_bins), p(cum), capacity, p(longest), s)
        staged = ids.clone()
        ops._call("ts_bin_gather_groups", lib.ts_bin_gather_groups, n, nt, p(bin_ws), p(tile_bins), p(bucket_ids), p(ids), s)
    elif form == GROUP:
        ops._call("ts_bin_count_groups", lib.ts_bin_count_groups, n, p(xys), p(rad), tl, cam, p(bin_ws), s)
        b, g = chunks(n)[0], (nt + 31) // 32
        matrix = bin_ws[:b * g].view(b, g).cpu()                  # pairs per (chunk, group), before they become bases
        ops._call("ts_group_offsets", lib.ts_group_offsets, n, nt, p(bin_ws), p(tile_bins), p(cum), capacity, p(longest), s)
        ops._call("ts_bin_scatter_groups", lib.ts_bin_scatter_groups, n, p(xys), p(rad), tl, cam, p(bin_ws), p(tile_bins),
                  p(bucket_ids), p(ids), s)
        staged = ids.clone()
    else:
        assert form == MATRIX
        ops._call("ts_bin_count", lib.ts_bin_count, n, p(xys), p(rad), tl, cam, p(bin_ws), s)
        ops._call("ts_tile_offsets_stats", lib.ts_tile_offsets_stats, n, nt, p(bin_ws), p(tile_bins), p(cum), capacity,
                  p(longest), s)
        ops._call("ts_bin_scatter", lib.ts_bin_scatter, n, p(xys), p(rad), tl, cam, p(bin_ws), p(bucket_ids), p(ids), s)
        staged = ids.clone()
    scattered = bucket_ids.clone()
    if form == MATRIX:
        ops._call("ts_sort_tiles", lib.ts_sort_tiles, nt, p(tile_bins), p(depths), p(bucket_ids), p(ids), p(bin_ws),
                  spare, s)
    else:
        ops._call("ts_sort_tiles_stats", lib.ts_sort_tiles_stats, nt, p(tile_bins), p(depths), p(bucket_ids), p(ids),
                  p(bin_ws), spare, n, p(bin_ws), p(longest), s)
    torch.cuda.synchronize()
    bins = tile_bins.cpu()
    listed = int(bins[:, 1].max())
    assert 0 <= listed <= total
    # tile_start[0..T] | guard | spare.  (ts_sort_tiles counts the lists beyond 4096 entries in the spare word: it is
    # compared as it stands after the sort in every form)
    tail = bin_ws[-(nt + 3):].cpu()
    return dict(bins=bins, ids=ids[:listed].cpu(), tail=tail, longest=int(longest), listed=listed, nt=nt,
                scattered=scattered.cpu(), staged=staged.cpu(), lens=(bins[:, 1] - bins[:, 0]), matrix=matrix)


def same(ref, got):
    assert torch.equal(ref["bins"], got["bins"])
    assert ref["listed"] == got["listed"] and torch.equal(ref["ids"], got["ids"])
    assert torch.equal(ref["tail"], got["tail"])            # tile_start[0..T], guard word, spare word
    assert int(ref["tail"][-2]) == 0
    want = int(ref["lens"].max())
    assert ref["longest"] == want and got["longest"] == want
    # the scatter filled exactly the listed part of bucket_ids (the order inside a bucket is arbitrary until the sort)
    for r in (ref, got):
        assert int(r["scattered"][:r["listed"]].min()) >= 0 and bool((r["scattered"][r["listed"]:] == SENTINEL).all())
