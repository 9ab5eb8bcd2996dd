"""GROUP COUNTS (csrc/binning.hip, frame.GROUP_COUNTS): a frame whose scatter runs in two hops counts its pairs per
(chunk, group of 32 lists) and the fine hop counts the lists themselves.  The lists are the same lists: stage by stage
through the C ABI against the matrix-form entries (ts_bin_count -> ts_tile_offsets_stats -> ts_bin_scatter ->
ts_sort_tiles), and frame against frame in one process with the switch on and off.  Everything is compared bit for bit.

n = 2^18 + 77 sits just above the two-hop threshold with a ragged last chunk; 400 x 304 is 25 x 19 = 475 tiles, i.e. 14
full groups and one of 27 tiles; a group's region is ~22 k entries (more than two fine passes) on the uniform scene and
several tens of fine passes on the clustered one."""
import ctypes

import pytest
import torch

from tinysplat_amd import _lib, frame, ops
from tinysplat_amd.rasterizer import project_args, tile_bounds
from tinysplat_amd.synthetic import make_scene

from test_gpu_survivors import _render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = (1 << 18) + 77
W, H = 400, 304
SENTINEL = -1
UNSET = -7
_scenes = {}


def _projected(clustered=0.0, n=N, tile_rows=None):
    """2-D inputs of the binning stages (projection, scan, packed records for the tight lists), once per scene"""
    key = (clustered, n, tile_rows)
    if key not in _scenes:
        lib = _lib.load()
        dev = torch.device(DEV)
        model, cam = make_scene(n, 0, W, H, seed=41, clustered=clustered)
        md = model.to(dev)
        with torch.no_grad():
            xys, depths, radii, conics, nth, _ = ops.project_gaussians(*project_args(md, cam, (W, H), DEV),
                                                                       tile_rows=tile_rows)
            opac = torch.sigmoid(md.opacities).reshape(-1).contiguous()
        colors = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(dev)
        i32 = dict(dtype=torch.int32, device=dev)
        s, p = ops._stream(dev), ops._ptr
        cum = torch.empty((n,), **i32)
        ws = torch.empty((int(lib.ts_scan_ws_ints(n)),), **i32)
        ops._call("ts_scan_tiles", lib.ts_scan_tiles, n, p(nth), p(cum), p(ws), None, s)
        splats = torch.zeros((n, 12), dtype=torch.float32, device=dev)
        cam16 = ops._camera(0.0, 0.0, 0.0, 0.0, H, W, tile_bounds((W, H)), tile_rows=tile_rows)
        ops._call("ts_pack_splats", lib.ts_pack_splats, n, 3, 0, p(xys), p(radii), p(conics), p(colors), p(opac), p(cum),
                  cam16, None, p(splats), s)
        torch.cuda.synchronize()
        _scenes[key] = dict(n=n, xys=xys, depths=depths, radii=radii, cum=cum, splats=splats, total=int(cum[-1]),
                            tile_rows=tile_rows)
    return _scenes[key]


def _chain(inp, group, wide=False, hints=0, capacity=-1):
    """the four list-building stages in one form -> everything a later stage or the host reads"""
    lib = _lib.load()
    dev = torch.device(DEV)
    n, total = inp["n"], inp["total"]
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, H, W, tile_bounds((W, H)), tile_rows=inp["tile_rows"], wide_tiles=wide)
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
    if group:
        ops._call("ts_bin_count_groups", lib.ts_bin_count_groups, n, p(xys), p(rad), tl, cam, p(bin_ws), s)
        ops._call("ts_group_offsets", lib.ts_group_offsets, n, nt, p(bin_ws), p(tile_bins), p(cum), capacity, p(longest), s)
        ops._call("ts_bin_scatter_groups", lib.ts_bin_scatter_groups, n, p(xys), p(rad), tl, cam, p(bin_ws), p(tile_bins),
                  p(bucket_ids), p(ids), s)
        scattered = bucket_ids.clone()
        ops._call("ts_sort_tiles_stats", lib.ts_sort_tiles_stats, nt, p(tile_bins), p(depths), p(bucket_ids), p(ids),
                  p(bin_ws), spare, n, p(bin_ws), p(longest), s)
    else:
        ops._call("ts_bin_count", lib.ts_bin_count, n, p(xys), p(rad), tl, cam, p(bin_ws), s)
        ops._call("ts_tile_offsets_stats", lib.ts_tile_offsets_stats, n, nt, p(bin_ws), p(tile_bins), p(cum), capacity,
                  p(longest), s)
        ops._call("ts_bin_scatter", lib.ts_bin_scatter, n, p(xys), p(rad), tl, cam, p(bin_ws), p(bucket_ids), p(ids), s)
        scattered = bucket_ids.clone()
        ops._call("ts_sort_tiles", lib.ts_sort_tiles, nt, p(tile_bins), p(depths), p(bucket_ids), p(ids), p(bin_ws),
                  spare, s)
    torch.cuda.synchronize()
    bins = tile_bins.cpu()
    listed = int(bins[:, 1].max())
    assert 0 <= listed <= total
    # tile_start[0..T] | guard | spare.  (ts_sort_tiles counts the lists beyond 4096 entries in the spare word: it is
    # compared as it stands after the sort in both forms)
    tail = bin_ws[-(nt + 3):].cpu()
    return dict(bins=bins, ids=ids[:listed].cpu(), tail=tail, longest=int(longest), listed=listed, nt=nt,
                scattered=scattered.cpu(), lens=(bins[:, 1] - bins[:, 0]))


def _same(ref, got):
    assert torch.equal(ref["bins"], got["bins"])
    assert ref["listed"] == got["listed"] and torch.equal(ref["ids"], got["ids"])
    assert torch.equal(ref["tail"], got["tail"])            # tile_start[0..T], guard word, spare word
    assert int(ref["tail"][-2]) == 0
    want = int(ref["lens"].max())
    assert ref["longest"] == want and got["longest"] == want
    # the scatter filled exactly the listed part of bucket_ids (the order inside a bucket is arbitrary until the sort)
    for r in (ref, got):
        assert int(r["scattered"][:r["listed"]].min()) >= 0 and bool((r["scattered"][r["listed"]:] == SENTINEL).all())


def test_predicate_and_refusals():
    lib = _lib.load()
    assert lib.ts_bin_group_form(N) == 1 and lib.ts_bin_group_form(1 << 18) == 1
    assert lib.ts_bin_group_form((1 << 18) - 1) == 0 and lib.ts_bin_group_form(0) == 0
    assert lib.ts_bin_group_form((1 << 27) - 1) == 1 and lib.ts_bin_group_form(1 << 27) == 0
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, H, W, tile_bounds((W, H)))
    # an n of the matrix form is refused before anything is launched (the pointers are never looked at)
    assert lib.ts_bin_count_groups((1 << 18) - 1, 8, 8, None, cam, 8, None) == -1
    assert lib.ts_group_offsets((1 << 18) - 1, 475, 8, 8, None, -1, None, None) == -1
    assert lib.ts_bin_scatter_groups((1 << 18) - 1, 8, 8, None, cam, 8, 8, 8, 8, None) == -1
    assert lib.ts_bin_scatter_groups(N, 8, 8, None, cam, 8, 8, 8, None, None) == -1          # no scratch: no two hops


def test_uniform_scene():
    inp = _projected()
    ref, got = _chain(inp, False), _chain(inp, True)
    assert ref["nt"] == 475
    per_group = ref["listed"] / 15
    print(f"[groups] uniform: listed {ref['listed']}, mean list {ref['listed'] / 475:.0f}, mean region {per_group:.0f}")
    assert per_group > 2 * 8192                               # more than two fine passes per region
    _same(ref, got)


def test_clustered_scene():
    inp = _projected(clustered=0.8)
    ref, got = _chain(inp, False), _chain(inp, True)
    lens = ref["lens"]
    regions = torch.nn.functional.pad(lens, (0, 480 - 475)).view(15, 32).sum(1)
    print(f"[groups] clustered: listed {ref['listed']}, longest {int(lens.max())}, empty lists {int((lens == 0).sum())}, "
          f"regions {regions.tolist()}")
    assert int(lens.max()) > 1024
    assert int(regions.max()) > 4 * 8192 and int(regions.min()) <= 8192      # many fine passes, and regions of a single one
    _same(ref, got)


def test_empty_lists_and_empty_groups():
    """every Gaussian inside the cluster window: most lists and whole groups are empty - and a group whose region is
    empty must still publish its (0, 0) lists and its tile starts"""
    inp = _projected(clustered=1.0)
    ref, got = _chain(inp, False), _chain(inp, True)
    regions = torch.nn.functional.pad(ref["lens"], (0, 480 - 475)).view(15, 32).sum(1)
    print(f"[groups] all clustered: regions {regions.tolist()}")
    assert int((regions == 0).sum()) > 0 and int((ref["lens"] == 0).sum()) > 32
    _same(ref, got)


def test_wide_lists():
    inp = _projected()
    ref, got = _chain(inp, False, wide=True), _chain(inp, True, wide=True)
    assert ref["nt"] == 13 * 19
    _same(ref, got)


def test_balanced_walk():
    inp = _projected()
    ref, got = _chain(inp, False, hints=1), _chain(inp, True, hints=1)      # TS_HINT_BALANCED_WALK
    _same(ref, got)
    _same(_chain(inp, False), got)


def test_stripe_camera():
    inp = _projected(tile_rows=(5, 12))
    ref, got = _chain(inp, False), _chain(inp, True)
    assert ref["nt"] == 7 * 25
    _same(ref, got)


def test_capacity_guard():
    inp = _projected()
    cap = inp["total"] - 1
    ref, got = _chain(inp, False, capacity=cap), _chain(inp, True, capacity=cap)
    for r in (ref, got):
        assert int(r["tail"][-2]) == 1                                       # the guard word
        assert int(r["bins"].abs().max()) == 0                               # every list (0, 0)
        assert bool((r["scattered"] == SENTINEL).all())                      # bucket_ids never touched
        assert int(r["tail"][:-2].abs().max()) == 0
        assert r["longest"] == UNSET                                         # nothing is stored for such a frame
    assert torch.equal(ref["tail"], got["tail"])
    fits = _chain(inp, True, capacity=inp["total"])                          # exactly enough: no guard
    _same(_chain(inp, False, capacity=inp["total"]), fits)


def _frames(n, depth):
    model, cam = make_scene(n, 1, W, H, seed=43)
    saved = (frame.GROUP_COUNTS, frame.WIDE_TILES)
    res, flags, words = [], [], []
    try:
        frame.WIDE_TILES = 0
        for on in (False, True, True):
            frame.GROUP_COUNTS = on
            out, F = _render(model, cam, (W, H), 1, depth)
            b = frame.last_binning[0]
            bins = b.tile_bins.clone()
            res.append(out + [bins, b.gaussian_ids_sorted[:int(bins[:, 1].max())].clone()])
            flags.append(bool(F.fr.flags & 1024))
            words.append((ctypes.c_int32.from_address(frame._pinned_total[0][0].data_ptr() + 4).value,
                          int((bins[:, 1] - bins[:, 0]).max())))
    finally:
        frame.GROUP_COUNTS, frame.WIDE_TILES = saved
    assert flags == [False, True, True]
    for word, want in words:                                  # the longest-list word of TS_FRAME_LIST_STATS
        assert word == want > 0
    assert len(res[0]) == (12 if depth else 11)               # image, final state[, depth], xys.grad, six parameters, lists
    for a, b, c in zip(*res):
        assert a.shape == b.shape and torch.equal(a, b)       # group form == matrix form
        assert torch.equal(b, c)                              # and the group form repeats itself
    return res


@pytest.mark.parametrize("depth", [False, True])
def test_frame_bitwise(depth):
    assert _lib.load().ts_bin_group_form(N) == 1
    res = _frames(N, depth)
    assert float(res[0][0].max()) > 0.1


def test_below_the_threshold_the_flag_changes_nothing():
    n = (1 << 18) - 1
    assert _lib.load().ts_bin_group_form(n) == 0
    _frames(n, True)
