"""ONE WALK (csrc/binning.hip, frame.ONE_WALK): a group-form frame builds its lists from one walk of the Gaussians - every
chunk stages its pairs in LDS, writes them into its own bounding-box slots of the scratch buffer, and the fine hop gathers
a group's runs.  The lists are the same lists: stage by stage through the C ABI against the group-form entries
(ts_bin_count_groups -> ts_group_offsets -> ts_bin_scatter_groups -> ts_sort_tiles_stats) on the same inputs, and frame
against frame in one process with the switch on and off.  Everything is compared bit for bit.

Shapes of tests/test_gpu_group_counts.py: n = 2^18 + 77 (193 chunks of 1359 Gaussians, a ragged last one), 400 x 304 =
475 tiles in 14 full groups and one of 27."""
import ctypes

import pytest
import torch

from tinysplat_amd import _lib, frame, ops
from tinysplat_amd.rasterizer import tile_bounds
from tinysplat_amd.synthetic import make_scene

from binning_cases import GROUP, H, N, SENTINEL, UNSET, W, WALK, chunks as _chunks, projected as _projected, same as _same
import binning_cases
from test_gpu_survivors import _render

pytestmark = pytest.mark.gpu


def _chain(inp, walk, **kw):
    return binning_cases.chain(inp, WALK if walk else GROUP, **kw)


def _rows_fit_their_slots(inp, ref):
    """the property the layout rests on: a chunk lists at most as many pairs as its Gaussians have bounding-box slots"""
    b, per = _chunks(N)
    cum = torch.cat([torch.zeros(1, dtype=torch.int64), inp["cum"].cpu().long()])
    edges = torch.tensor([min(N, k * per) for k in range(b + 1)])
    room = cum[edges[1:]] - cum[edges[:-1]]
    rows = ref["matrix"].long().sum(1)
    assert rows.shape == room.shape and bool((rows <= room).all())
    assert int(rows.sum()) == ref["listed"]
    return rows


def _pair(inp, **kw):
    ref, got = _chain(inp, False, **kw), _chain(inp, True, **kw)
    rows = _rows_fit_their_slots(inp, ref)
    _same(ref, got)
    return ref, got, rows


def test_predicate_and_refusals():
    lib = _lib.load()
    cap = lib.ts_bin_stage_capacity()
    assert 1024 <= cap and 6 * cap <= 144 * 1024
    assert lib.ts_bin_one_walk_form(N, 475) == 1 and lib.ts_bin_one_walk_form(1 << 18, 8160) == 1
    assert lib.ts_bin_one_walk_form((1 << 18) - 1, 475) == 0 and lib.ts_bin_one_walk_form(1 << 27, 475) == 0
    assert lib.ts_bin_one_walk_form(N, 0) == 0 and lib.ts_bin_one_walk_form(N, 1) == 0
    assert lib.ts_bin_one_walk_form(N, 32 * 2048) == 1 and lib.ts_bin_one_walk_form(N, 32 * 2048 + 1) == 0
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, H, W, tile_bounds((W, H)))
    # an n of the matrix form is refused before anything is launched (the pointers are never looked at)
    small = (1 << 18) - 1
    assert lib.ts_bin_emit_groups(small, 8, 8, None, cam, 8, -1, 8, 8, None) == -1
    assert lib.ts_emit_offsets(small, 475, 8, 8, 8, -1, None, None) == -1
    assert lib.ts_bin_gather_groups(small, 475, 8, 8, 8, 8, None) == -1
    cam.hints = 1                                                            # TS_HINT_BALANCED_WALK: the group form's frame
    assert lib.ts_bin_emit_groups(N, 8, 8, None, cam, 8, -1, 8, 8, None) == -1


def test_uniform_scene():
    inp = _projected()
    ref, got, rows = _pair(inp)
    assert ref["nt"] == 475
    print(f"[one walk] uniform: listed {ref['listed']}, pairs per chunk {int(rows.min())}..{int(rows.max())}")
    assert int(rows.max()) <= _lib.load().ts_bin_stage_capacity()            # every chunk staged


def test_clustered_scene():
    inp = _projected(clustered=0.8)
    ref, got, rows = _pair(inp)
    print(f"[one walk] clustered: listed {ref['listed']}, longest {int(ref['lens'].max())}, "
          f"pairs per chunk {int(rows.min())}..{int(rows.max())}")
    assert int(ref["lens"].max()) > 1024


def test_staged_and_twice_walked_chunks():
    """the first half of the Gaussians enlarged 24 times: their chunks list more than the staging buffer holds and walk
    twice, the others stage - asserted from the group form's count matrix and the exported capacity"""
    cap = _lib.load().ts_bin_stage_capacity()
    inp = _projected(enlarge=(0.5, 24.0))
    ref, got, rows = _pair(inp)
    over, fit = int((rows > cap).sum()), int(((rows <= cap) & (rows > 0)).sum())
    print(f"[one walk] enlarged: listed {ref['listed']}, pairs per chunk {int(rows.min())}..{int(rows.max())}, "
          f"capacity {cap}: {over} chunks walk twice, {fit} stage")
    assert over >= 8 and fit >= 8


def test_empty_lists_and_empty_groups():
    inp = _projected(clustered=1.0)
    ref, got, rows = _pair(inp)
    regions = torch.nn.functional.pad(ref["lens"], (0, 480 - 475)).view(15, 32).sum(1)
    assert int((regions == 0).sum()) > 0 and int((ref["lens"] == 0).sum()) > 32


def test_wide_lists():
    ref, got, rows = _pair(_projected(), wide=True)
    assert ref["nt"] == 13 * 19


def test_stripe_camera():
    ref, got, rows = _pair(_projected(tile_rows=(5, 12)))
    assert ref["nt"] == 7 * 25


def test_column_scan_launch():
    """2400 x 2400: 22 500 tiles in 704 groups - 193 x 704 counts are more than one workgroup scans, the column-scan
    launch runs in front of the offsets"""
    ref, got, rows = _pair(_projected(dims=(2400, 2400)))
    assert ref["nt"] == 22500 and _chunks(N)[0] * 704 > (1 << 17)


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
    assert bool((got["staged"] == SENTINEL).all())                           # nor scratch: the emit launch checks by itself
    assert torch.equal(ref["tail"], got["tail"])
    _same(_chain(inp, False, capacity=inp["total"]), _chain(inp, True, capacity=inp["total"]))     # exactly enough


def test_two_runs_agree():
    inp = _projected(clustered=0.8)
    a, b = _chain(inp, True), _chain(inp, True)
    for k in ("bins", "ids", "tail"):
        assert torch.equal(a[k], b[k])
    assert a["longest"] == b["longest"]


def _frames(n, depth, balanced=False):
    """the frame with the switch off, on, on -> results, and the entries the executor issued for each"""
    lib = _lib.load()
    model, cam = make_scene(n, 1, W, H, seed=43)
    saved = (frame.ONE_WALK, frame.WIDE_TILES, frame.BALANCED_WALK_FROM)
    res, flags, issued = [], [], []
    seen = []
    probe = _lib.ENTRY_PROBE(lambda entry, end, user: seen.append(entry.decode()) if not end else None)
    try:
        frame.WIDE_TILES = 0
        if balanced:
            frame.BALANCED_WALK_FROM = 0.0                        # every frame behind the first one carries the hint
            _render(model, cam, (W, H), 1, depth)
        for on in (False, True, True):
            frame.ONE_WALK = on
            del seen[:]
            assert lib.ts_set_entry_probe(probe, None) == 0
            try:
                out, F = _render(model, cam, (W, H), 1, depth)
            finally:
                assert lib.ts_set_entry_probe(None, None) == 0
            b = frame.last_binning[0]
            bins = b.tile_bins.clone()
            res.append(out + [bins, b.gaussian_ids_sorted[:int(bins[:, 1].max())].clone()])
            flags.append(bool(F.fr.flags & 2048))
            issued.append(list(seen))
            assert bool(F.fr.cam.hints & 1) == balanced
            word = ctypes.c_int32.from_address(frame._pinned_total[0][0].data_ptr() + 4).value
            assert word == int((bins[:, 1] - bins[:, 0]).max()) > 0          # the longest-list word of TS_FRAME_LIST_STATS
    finally:
        frame.ONE_WALK, frame.WIDE_TILES, frame.BALANCED_WALK_FROM = saved
    assert flags == [False, True, True]
    assert len(res[0]) == (12 if depth else 11)               # image, final state[, depth], xys.grad, six parameters, lists
    for a, b, c in zip(*res):
        assert a.shape == b.shape and torch.equal(a, b)       # one walk == group form
        assert torch.equal(b, c)                              # and repeats itself
    return res, issued


@pytest.mark.parametrize("depth", [False, True])
def test_frame_bitwise(depth):
    assert _lib.load().ts_bin_one_walk_form(N, 475) == 1
    res, issued = _frames(N, depth)
    assert float(res[0][0].max()) > 0.1
    assert "ts_bin_count" in issued[0]
    for run in issued[1:]:                                    # emit, offsets, fine hop: no count launch, offsets behind the emit
        assert "ts_bin_count" not in run
        k = run.index("ts_tile_offsets")
        assert run[k - 1] == "ts_bin_scatter" and run[k + 1] == "ts_bin_scatter" and run[k + 2] == "ts_sort_tiles"


def test_below_the_threshold_the_flag_changes_nothing():
    n = (1 << 18) - 1
    assert _lib.load().ts_bin_group_form(n) == 0
    res, issued = _frames(n, True)
    assert issued[0] == issued[1] == issued[2] and "ts_bin_count" in issued[1]


def test_with_the_balanced_walk_hint_the_flag_changes_nothing():
    res, issued = _frames(N, True, balanced=True)
    assert issued[0] == issued[1] == issued[2] and "ts_bin_count" in issued[1]
