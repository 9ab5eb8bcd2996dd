"""Every form of the per-tile depth sort at its length boundaries, against a host order (tests/sort_cases.py; what each
list reaches is shown without a GPU by tests/test_sort_cases_cpu.py).

The separate sorts - ts_sort_tiles, ts_sort_tiles_stats, ts_sort_tiles_above - run on 38 lists of 0 .. 200 000 entries:
one wave's register network (E = 1 .. 16), the workgroup network (E = 1 .. 16), and the sample sort with its three ways
to sort a sub-bucket, the global-memory network included (bucket order "samples first").  The sorts inside the forward
compositing launch - ts_raster_fwd_sort: the one-wave mapping, wave 0 of the split mapping, the cooperative tiles' four
runs and their merge - run on a 123 x 89 frame that holds every in-kernel length twice, and the launch is compared with
ts_raster_fwd_planes on the host-sorted lists.  Everything through the C ABI, every comparison bit for bit; a failure
names the lengths of the lists that are out of order.

(ts_raster_fwd_sort composites a list in the launch that sorts it: a network that drops keys leaves the low word of its
padding keys, -1, in the list, and the launch reads the record in front of the array before any assertion here can
look at the list.  Try a change to the in-launch sorts on the separate sorts' dispatch first - they share
sort_tile_wave - where a wrong list is only compared.)"""
import ctypes

import numpy as np
import pytest
import torch

import sort_cases as S
from tinysplat_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 1024                      # sentinel words behind the listed part of every id buffer
UNSET = -7
_dev = {}


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _padded(ids):
    return _i32(np.concatenate([ids, np.full(PAD, S.SENTINEL, dtype=np.int32)]))


def _device(c, name):
    if name not in _dev:
        _dev[name] = dict(bins=_i32(c["tile_bins"]), depths=_f32(c["depths"]), bucket=_padded(c["bucket_ids"]))
        assert torch.equal(_dev[name]["depths"].cpu().view(torch.int32),
                           torch.from_numpy(c["depths"]).view(torch.int32))     # no bit of an edge pattern lost
    return _dev[name]


def _out(c):
    return torch.full((c["listed"] + PAD,), S.SENTINEL, dtype=torch.int32, device=DEV)


def _check_lists(c, got, which=lambda n: True, note=lambda t: ""):
    bad = [f"{n}{note(t)}" for t, n, sl in S.tile_slices(c) if which(n) and not np.array_equal(got[sl], c["expect"][sl])]
    assert not bad, f"lists of these lengths are not in host order: {', '.join(bad)}"


def _separate_sort(c, d, entry, out, ws, zeroed):
    """one of the three-launch sorts -> (ids buffer, counter word)"""
    lib = _lib.load()
    nt = len(c["lens"])
    s, p = ops._stream(torch.device(DEV)), ops._ptr
    word = torch.zeros((1,), dtype=torch.int32, device=DEV) if zeroed else None
    if entry == "ts_sort_tiles":
        ops._call(entry, lib.ts_sort_tiles, nt, p(d["bins"]), p(d["depths"]), p(d["bucket"]), p(out), p(ws), p(word), s)
    else:                                   # longest_list = NULL: n and bin_ws are ignored
        ops._call(entry, lib.ts_sort_tiles_stats, nt, p(d["bins"]), p(d["depths"]), p(d["bucket"]), p(out), p(ws), p(word),
                  0, None, None, s)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(word if zeroed else ws[0])


@pytest.mark.parametrize("order", S.ORDERS)
@pytest.mark.parametrize("population", S.POPULATIONS)
def test_separate_sort(population, order):
    c = S.case(population, order)
    d = _device(c, ("case", population, order))
    nt, listed = len(c["lens"]), c["listed"]
    beyond = int((c["lens"] > S.SORT_CAP).sum())
    assert beyond == 11
    first = None
    for entry, zeroed in (("ts_sort_tiles", False), ("ts_sort_tiles", True), ("ts_sort_tiles_stats", False),
                          ("ts_sort_tiles_stats", True)):
        out, ws = _out(c), torch.full((nt + 1,), UNSET, dtype=torch.int32, device=DEV)
        got, counter = _separate_sort(c, d, entry, out, ws, zeroed)
        _check_lists(c, got)
        assert np.array_equal(got[:listed], c["expect"])
        assert (got[listed:] == S.SENTINEL).all()                            # nothing written beyond the lists
        assert counter == beyond                                             # the lists beyond kSortCap, queued once each
        if first is None:
            first = got
            # a second call on the same buffers: no atomics in the result, the queue's order does not show
            again, counter = _separate_sort(c, d, entry, out, ws, zeroed)
            assert np.array_equal(again, first) and counter == beyond
    bucket = d["bucket"].cpu().numpy()
    assert np.array_equal(bucket[:listed], c["bucket_ids"]) and (bucket[listed:] == S.SENTINEL).all()


@pytest.mark.parametrize("order", S.ORDERS)
@pytest.mark.parametrize("population", S.POPULATIONS)
def test_sort_above_leaves_the_short_lists(population, order):
    """ts_sort_tiles_above (one launch, the sample sort on the workgroup's own 48 KiB): the lists above 1024 entries in
    host order, the range of every shorter list untouched - those belong to ts_raster_fwd_sort"""
    lib = _lib.load()
    c = S.case(population, order)
    d = _device(c, ("case", population, order))
    s, p = ops._stream(torch.device(DEV)), ops._ptr
    out = _out(c)
    first = None
    for _ in range(2):
        ops._call("ts_sort_tiles_above", lib.ts_sort_tiles_above, len(c["lens"]), p(d["bins"]), p(d["depths"]),
                  p(d["bucket"]), p(out), None, None, s)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _check_lists(c, got, lambda n: n > S.WAVE_SORT_MAX)
        touched = [n for _, n, sl in S.tile_slices(c) if n <= S.WAVE_SORT_MAX and (got[sl] != S.SENTINEL).any()]
        assert not touched, f"lists of these lengths were written: {touched}"
        assert (got[c["listed"]:] == S.SENTINEL).all()
        first = got if first is None else first
        assert np.array_equal(got, first)
    assert np.array_equal(d["bucket"].cpu().numpy()[:c["listed"]], c["bucket_ids"])


# ---- the sorts inside the forward compositing launch -----------------------------------------------------------------
MAPPINGS = {"whole": (0, 0),                                                 # one wave per tile sorts its list
            "split": (_lib.RASTER_SPLIT_BLOCKS, 0),                          # a workgroup per tile, wave 0 sorts
            "coop split": (_lib.RASTER_SPLIT_BLOCKS, _lib.HINT_COOP_SPLIT),  # every tile cooperative: four runs, merged
            "coop band": (0, S.FRAME_COOP16 << 16)}                          # TS_CAM_COOP_TILES(8): half of every band
_refs = {}


def _camera(hints):
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, S.FRAME_H, S.FRAME_W, (S.FRAME_TBX, S.FRAME_TBY, 1))
    cam.hints = hints
    assert _lib.load().ts_num_tiles(ctypes.byref(cam)) == S.FRAME_TILES
    return cam


def _frame(population, channels):
    """the frame's lists and the packed records of its Gaussians on the device"""
    key = ("frame", population, channels)
    if key not in _dev:
        lib = _lib.load()
        c = S.frame_case(population)
        d = dict(_device(c, ("frame lists", population)))
        d["sorted"] = _padded(c["expect"])
        n = S.FRAME_POOL
        col = _f32(c["colors"] if channels == 4 else c["colors"][:, :3])
        xys, conics, opac, radii, cum = _f32(c["xys"]), _f32(c["conics"]), _f32(c["opacity"]), _i32(c["radii"]), _i32(c["cum"])
        d["splats"] = torch.zeros((n, 12), dtype=torch.float32, device=DEV)
        s, p = ops._stream(torch.device(DEV)), ops._ptr
        ops._call("ts_pack_splats", lib.ts_pack_splats, n, channels, 0, p(xys), p(radii), p(conics), p(col), p(opac), p(cum),
                  _camera(0), None, p(d["splats"]), s)
        torch.cuda.synchronize()
        assert bool((d["splats"][:, 2] == opac).all())                       # every Gaussian was packed
        d["bg"] = _f32(np.array([0.1, 0.2, 0.3, 0.4][:channels]))
        _dev[key] = d
    return _dev[key]


def _launch(population, channels, mapping, ids=None, fill=7.0):
    """ts_raster_fwd_planes on the lists `ids`, or (ids = None) ts_sort_tiles_above + ts_raster_fwd_sort on the buckets
    -> everything the launch wrote, on the host"""
    lib = _lib.load()
    c, d = S.frame_case(population), _frame(population, channels)
    flags, hints = MAPPINGS[mapping]
    cam = _camera(hints)
    h, w = S.FRAME_H, S.FRAME_W
    assert lib.ts_final_floats(ctypes.byref(cam), channels) == h * w
    img = torch.full((h, w, 3), fill, dtype=torch.float32, device=DEV)
    depth = torch.full((h, w), fill, dtype=torch.float32, device=DEV) if channels == 4 else None
    ts = torch.full((h, w), fill, dtype=torch.float32, device=DEV)
    idx = torch.full((h, w), int(fill) - 100, dtype=torch.int32, device=DEV)
    s, p = ops._stream(torch.device(DEV)), ops._ptr
    out = None
    if ids is not None:
        ops._call("ts_raster_fwd_planes", lib.ts_raster_fwd_planes, channels, flags, cam, p(d["bins"]), p(ids),
                  p(d["splats"]), p(d["bg"]), p(img), p(depth), p(ts), p(idx), None, s)
    else:
        out = _out(c)
        ops._call("ts_sort_tiles_above", lib.ts_sort_tiles_above, S.FRAME_TILES, p(d["bins"]), p(d["depths"]),
                  p(d["bucket"]), p(out), None, None, s)
        ops._call("ts_raster_fwd_sort", lib.ts_raster_fwd_sort, channels, flags, cam, p(d["bins"]), p(d["bucket"]),
                  p(d["depths"]), p(out), p(d["splats"]), p(d["bg"]), p(img), p(depth), p(ts), p(idx), None, s)
    torch.cuda.synchronize()
    return dict(img=img.cpu(), depth=None if depth is None else depth.cpu(), Ts=ts.cpu(), idx=idx.cpu(),
                ids=None if out is None else out.cpu().numpy())


def _tile(a, t):
    ty, tx = divmod(t, S.FRAME_TBX)
    return a[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]


def _reference(population, channels, mapping):
    """the mapping's launch on the host-sorted lists, and the two conditions that keep a comparison with it from being
    empty: the lists of up to 1024 entries are walked to their end, and the order of a list shows in the picture"""
    key = (population, channels, mapping)
    if key not in _refs:
        c, d = S.frame_case(population), _frame(population, channels)
        ref = _launch(population, channels, mapping, ids=d["sorted"])
        unsorted = _launch(population, channels, mapping, ids=d["bucket"])
        for t, n, sl in S.tile_slices(c):
            if n <= S.WAVE_SORT_MAX:
                assert bool((_tile(ref["idx"], t) == sl.stop - 1).any()), f"the list of {n} entries is not walked to its end"
            if n >= 65:
                assert not torch.equal(_tile(ref["img"], t), _tile(unsorted["img"], t)), f"order of {n} entries: same image"
        assert bool(torch.isfinite(ref["img"]).all()) and bool((ref["Ts"] > 0).all())
        _refs[key] = ref
    return _refs[key]


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("population", S.FRAME_POPULATIONS)
def test_sort_inside_the_forward_launch(population, channels, mapping):
    c = S.frame_case(population)
    ref = _reference(population, channels, mapping)
    got = _launch(population, channels, mapping, fill=-3.0)
    coop = np.ones(S.FRAME_TILES, dtype=bool) if mapping == "coop split" else \
        c["coop"] if mapping == "coop band" else np.zeros(S.FRAME_TILES, dtype=bool)
    _check_lists(c, got["ids"], note=lambda t: " (cooperative tile)" if coop[t] else "")
    assert np.array_equal(got["ids"][:c["listed"]], c["expect"]) and (got["ids"][c["listed"]:] == S.SENTINEL).all()
    for name in ("img", "depth", "Ts", "idx"):
        if ref[name] is not None:
            assert torch.equal(got[name], ref[name]), name
    whole = _reference(population, channels, "whole")                        # the images equal across mappings
    for name in ("img", "depth", "Ts", "idx"):
        if ref[name] is not None:
            assert torch.equal(ref[name], whole[name]), name
    d = _frame(population, channels)
    assert np.array_equal(d["bucket"].cpu().numpy()[:c["listed"]], c["bucket_ids"])
