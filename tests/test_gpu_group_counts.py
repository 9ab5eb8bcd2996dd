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
from tinysplat_amd.rasterizer import tile_bounds
from tinysplat_amd.synthetic import make_scene

from binning_cases import GROUP, H, MATRIX, N, SENTINEL, UNSET, W, projected as _projected, same as _same
import binning_cases
from test_gpu_survivors import _render

pytestmark = pytest.mark.gpu


def _chain(inp, group, **kw):
    return binning_cases.chain(inp, GROUP if group else MATRIX, **kw)


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
