"""ROW SPANS (csrc/row_spans.h, frame.ROW_SPANS): in a one-walk frame the colour stage leaves a 16-byte record per Gaussian
with the tile columns of every row of its box, and the emit launch walks the records instead of computing them.  The lists
are the same lists.  Three levels, everything compared bit for bit:

  stages   ts_colors_pack_spans_fwd -> ts_bin_emit_groups_spans -> ts_emit_offsets -> ts_bin_gather_groups -> sort against
           the one-walk entries without records (tests/binning_cases.py: chain) on the same 2-D inputs: tile_bins, the
           sorted ids, tile_start, guard, spare and longest-list words.  Inputs: the base set of binning_cases (uniform,
           clustered, 24x enlarged, empty groups, wide lists, a stripe with tile_row0 > 0 through the dense and the sparse
           colour kernel, the capacity guard) and inputs made for the record's edges (boxes of exactly six and seven
           rows in one chunk, 257 tile columns, a needle of ~40 tiles, opacities of sigmoid(-12), bounding-box lists,
           hand-made records with an empty row between two others, and chunks whose pairs - or pairs and staged
           runs - exceed the staging buffer)
  records  what the GPU writes equals the header's host build, word for word
  frames   the same frame with frame.ROW_SPANS off and on: image, final_Ts, final_index, the six gradients, tile_bins,
           sorted ids and the words behind the lists, RGB and RGB + depth

n = 2^18 + 77 (193 chunks of 1359 Gaussians; not a multiple of the colour stage's 128) on 400 x 304 = 475 tiles."""
import ctypes

import numpy as np
import pytest
import torch

from tinysplat_amd import _lib, frame, ops
from tinysplat_amd.rasterizer import project_args, tile_bounds
from tinysplat_amd.synthetic import make_scene

import binning_cases as B
import row_spans_cases as R
from binning_cases import DEV, H, N, SENTINEL, UNSET, W, WALK
from test_gpu_survivors import _render

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("row_spans"))


def _stripe(dims, tile_rows):
    tbx, tby = (dims[0] + 15) // 16, (dims[1] + 15) // 16
    return (tbx, tby) + ((tile_rows[0], tile_rows[1] - tile_rows[0]) if tile_rows else (0, tby))


def _box_tiles(xys, radii, dims, tile_rows):
    """num_tiles_hit as the projection counts it: ts::tile_bbox in float32, rows clipped to the stripe"""
    tbx, tby, row0, rows = _stripe(dims, tile_rows)
    c, r = xys / 16.0, (radii.float() / 16.0)[:, None]
    lo = torch.trunc(c - r).clamp_min(0.0)
    hi = torch.trunc(c + r + 1.0).clamp_min(0.0)
    minx, maxx = lo[:, 0].clamp_max(tbx).int(), hi[:, 0].clamp_max(tbx).int()
    miny, maxy = lo[:, 1].clamp_max(tby).int().clamp_min(row0), hi[:, 1].clamp_max(tby).int().clamp_max(row0 + rows)
    full = (maxx - minx) * (hi[:, 1].clamp_max(tby).int() - lo[:, 1].clamp_max(tby).int())
    cnt = (maxx - minx).clamp_min(0) * (maxy - miny).clamp_min(0)
    return torch.where((radii > 0) & (full > 0), cnt, torch.zeros_like(cnt)).int()


def _inputs(name, clustered=0.0, tile_rows=None, enlarge=None, dims=(W, H), craft=None):
    """the 2-D inputs of the stages, once per case.  craft(rng) -> (rows of the arrays to overwrite, xy, radius, conic,
    opacity): Gaussians placed by hand"""
    if name in _cache:
        return _cache[name]
    lib, dev = _lib.load(), torch.device(DEV)
    w, h = dims
    model, cam = make_scene(N, 0, w, h, seed=41, clustered=clustered)
    if enlarge:
        with torch.no_grad():
            model.scales[:int(N * enlarge[0])] += torch.log(torch.tensor(float(enlarge[1])))
    md = model.to(dev)
    with torch.no_grad():
        xys, depths, radii, conics, nth, _ = ops.project_gaussians(*project_args(md, cam, (w, h), DEV), tile_rows=tile_rows)
        opac = torch.sigmoid(md.opacities).reshape(-1).contiguous()
    if craft is not None:
        at, xy, rad, con, op = (torch.as_tensor(a).to(dev) for a in craft(np.random.default_rng(7)))
        xys[at], radii[at], conics[at], opac[at] = xy.float(), rad.int(), con.float(), op.float()
        untouched = torch.ones((N,), dtype=torch.bool, device=dev)
        untouched[at] = False
        box = _box_tiles(xys, radii, dims, tile_rows)
        assert torch.equal(box[untouched], nth[untouched])        # the projection's own count, where it was left alone
        nth = box
    s, p = ops._stream(dev), ops._ptr
    cum = torch.empty((N,), dtype=torch.int32, device=dev)
    ws = torch.empty((int(lib.ts_scan_ws_ints(N)),), dtype=torch.int32, device=dev)
    ops._call("ts_scan_tiles", lib.ts_scan_tiles, N, p(nth), p(cum), p(ws), None, s)
    colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    splats = torch.zeros((N, 12), dtype=torch.float32, device=dev)
    cam16 = ops._camera(0.0, 0.0, 0.0, 0.0, h, w, tile_bounds((w, h)), tile_rows=tile_rows)
    ops._call("ts_pack_splats", lib.ts_pack_splats, N, 3, 0, p(xys), p(radii), p(conics), p(colors), p(opac), p(cum),
              cam16, None, p(splats), s)
    torch.cuda.synchronize()
    _cache[name] = dict(n=N, xys=xys, depths=depths, radii=radii, conics=conics, opac=opac, nth=nth, cum=cum,
                        colors=colors, splats=splats, total=int(cum[-1]), tile_rows=tile_rows, dims=dims)
    return _cache[name]


def _colour_stage(inp, tight, sparse=False):
    """the colour stage with span records (degree 0: the dense kernel without coefficient rows, or the sparse kernel)
    -> spans [n, 4] int32, splats [n, 12]"""
    lib, dev = _lib.load(), torch.device(DEV)
    n, (w, h) = inp["n"], inp["dims"]
    s, p = ops._stream(dev), ops._ptr
    cam16 = ops._camera(0.0, 0.0, 0.0, 0.0, h, w, tile_bounds((w, h)), tile_rows=inp["tile_rows"])
    means = torch.zeros((n, 3), device=dev)
    means[:, 2] = 1.0
    origin = torch.zeros((3,), device=dev)
    spans = torch.full((n, 4), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    splats = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    ops._call("ts_colors_pack_spans_fwd", lib.ts_colors_pack_spans_fwd, n, 0, 1, p(means), p(origin), p(inp["colors"]),
              None, None, p(inp["nth"]) if sparse else None, 3, 0, p(inp["xys"]), p(inp["radii"]), p(inp["conics"]),
              p(inp["opac"]), p(inp["cum"]), cam16, None, p(splats), 1 if tight else 0, p(spans), s)
    torch.cuda.synchronize()
    return spans, splats


def _span_chain(inp, spans, splats, wide=False, capacity=-1, blind=False):
    """binning_cases.chain's one-walk branch with the records given -> the same dictionary.  blind: the walk gets zeroed
    xys, radii and records - it must not need them (no record may carry the fallback flag)"""
    lib, dev = _lib.load(), torch.device(DEV)
    n, total, (w, h) = inp["n"], inp["total"], inp["dims"]
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, h, w, tile_bounds((w, h)), tile_rows=inp["tile_rows"], wide_tiles=wide)
    nt = int(lib.ts_num_tiles(ctypes.byref(cam)))
    i32 = dict(dtype=torch.int32, device=dev)
    s, p = ops._stream(dev), ops._ptr
    xys, rad = inp["xys"], inp["radii"]
    if blind:
        xys, rad = torch.zeros_like(xys), torch.zeros_like(rad)
        splats = None if splats is None else torch.zeros_like(splats)
    bin_ws = torch.full((int(lib.ts_bin_ws_ints(n, nt)),), UNSET, **i32)
    tile_bins = torch.full((nt, 2), UNSET, **i32)
    bucket_ids = torch.full((total,), SENTINEL, **i32)
    ids = torch.full((total,), SENTINEL, **i32)
    longest = torch.full((1,), UNSET, **i32)
    spare = bin_ws.data_ptr() + 4 * (bin_ws.numel() - 1)
    assert lib.ts_bin_one_walk_form(n, nt) == 1
    ops._call("ts_bin_emit_groups_spans", lib.ts_bin_emit_groups_spans, n, p(xys), p(rad), p(splats), p(spans), cam,
              p(inp["cum"]), capacity, p(bin_ws), p(ids), s)
    ops._call("ts_emit_offsets", lib.ts_emit_offsets, n, nt, p(bin_ws), p(tile_bins), p(inp["cum"]), capacity, p(longest), s)
    staged = ids.clone()
    ops._call("ts_bin_gather_groups", lib.ts_bin_gather_groups, n, nt, p(bin_ws), p(tile_bins), p(bucket_ids), p(ids), s)
    scattered = bucket_ids.clone()
    ops._call("ts_sort_tiles_stats", lib.ts_sort_tiles_stats, nt, p(tile_bins), p(inp["depths"]), p(bucket_ids), p(ids),
              p(bin_ws), spare, n, p(bin_ws), p(longest), s)
    torch.cuda.synchronize()
    bins = tile_bins.cpu()
    listed = int(bins[:, 1].max())
    assert 0 <= listed <= total
    return dict(bins=bins, ids=ids[:listed].cpu(), tail=bin_ws[-(nt + 3):].cpu(), longest=int(longest), listed=listed,
                nt=nt, scattered=scattered.cpu(), staged=staged.cpu(), lens=(bins[:, 1] - bins[:, 0]), matrix=None)


def _check(host, inp, tight=True, wide=False, sparse=False):
    """spans from the colour stage == the host's; the lists walked from them == the lists computed by the walk"""
    spans, splats = _colour_stage(inp, tight, sparse)
    tbx, tby, row0, rows = _stripe(inp["dims"], inp["tile_rows"])
    recs = torch.cat([inp["xys"], inp["opac"][:, None], inp["conics"]], 1).cpu().numpy()      # the values as packed
    radii = inp["radii"].cpu().numpy()
    if sparse:                                                   # a Gaussian the stripe does not list is skipped unseen
        radii = np.where(inp["nth"].cpu().numpy() > 0, radii, 0)
    got = spans.cpu().numpy().view(np.uint32)
    want = R.host_spans(host, recs, radii, tight, tbx, tby, row0, rows)
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} records differ from the host's"
    st = R.check_against_loops(host, got, recs, radii, tight, tbx, tby, row0, rows)
    # the records the colour stage packs beside the spans are ts_pack_splats' (the words the tight test reads)
    listed = inp["nth"] > 0
    assert torch.equal(splats[listed][:, :6], inp["splats"][listed][:, :6])
    ref_inp = inp if tight else dict(inp, splats=None)
    ref = B.chain(ref_inp, WALK, wide=wide)
    walked = _span_chain(inp, spans, splats if tight else None, wide=wide, blind=st["fallback"] == 0)
    B.same(ref, walked)
    return st, ref, spans, splats


def test_entries_and_refusals():
    lib = _lib.load()
    assert _lib.FRAME_ROW_SPANS == 4096 and "TS_FRAME_ROW_SPANS (4096)" in (R.ROOT / "include" / "tinysplat_hip.h").read_text()
    assert lib.ts_frame_struct_bytes() == ctypes.sizeof(_lib.TsFrame)
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, H, W, tile_bounds((W, H)))
    assert lib.ts_bin_emit_groups_spans((1 << 18) - 1, 8, 8, None, 16, cam, 8, -1, 8, 8, None) == -1     # not a one-walk n
    assert lib.ts_bin_emit_groups_spans(N, 8, 8, None, 20, cam, 8, -1, 8, 8, None) == -1                 # records not aligned
    assert lib.ts_colors_pack_spans_fwd(4, 0, 1, *([8] * 6), 3, 0, *([8] * 5), cam, None, 16, 1, 20, None) == -1


def test_uniform_scene(host):
    st, ref, _, _ = _check(host, _inputs("uniform"))
    print(f"[row spans] uniform: rows per box {st['rows'].tolist()}, fallback {st['fallback']}, skipped {st['skipped']}, "
          f"empty rows {st['empty_rows']}, listed {ref['listed']}")
    assert st["fallback"] == 0 and st["rows"][1:3].min() > 0 and st["skipped"] > N // 20


def test_clustered_scene(host):
    st, ref, _, _ = _check(host, _inputs("clustered", clustered=0.8))
    assert int(ref["lens"].max()) > 1024


def test_staged_and_twice_walked_chunks(host):
    """24x enlarged Gaussians: chunks beyond the staging buffer walk the records twice; boxes beyond six rows fall back"""
    cap = _lib.load().ts_bin_stage_capacity()
    st, ref, _, _ = _check(host, _inputs("enlarged", enlarge=(0.5, 24.0)))
    rows = B.chain(_inputs("enlarged"), B.GROUP)["matrix"].long().sum(1)
    assert int((rows > cap).sum()) >= 8 and int(((rows <= cap) & (rows > 0)).sum()) >= 8
    assert st["fallback"] > 1000 and st["rows"][1:].min() > 0
    print(f"[row spans] enlarged: rows per box {st['rows'].tolist()}, fallback {st['fallback']}")


def test_empty_lists_and_empty_groups(host):
    st, ref, _, _ = _check(host, _inputs("one cluster", clustered=1.0))
    assert int((ref["lens"] == 0).sum()) > 32


def test_wide_lists(host):
    st, ref, _, _ = _check(host, _inputs("uniform"), wide=True)
    assert ref["nt"] == 13 * 19


@pytest.mark.parametrize("sparse", [False, True])
def test_stripe_camera(host, sparse):
    """tile_row0 = 5: the first row of a record counts from the stripe; the sparse kernel writes the empty record for
    a Gaussian it skips"""
    st, ref, spans, _ = _check(host, _inputs("stripe", tile_rows=(5, 12)), sparse=sparse)
    assert ref["nt"] == 7 * 25 and st["skipped"] > N // 3


def test_bounding_box_lists(host):
    st, ref, _, _ = _check(host, _inputs("uniform"), tight=False)
    assert st["empty_rows"] == 0
    tight = B.chain(_inputs("uniform"), WALK)
    assert ref["listed"] > tight["listed"]


def test_capacity_guard(host):
    inp = _inputs("uniform")
    spans, splats = _colour_stage(inp, True)
    cap = inp["total"] - 1
    ref, got = B.chain(inp, WALK, capacity=cap), _span_chain(inp, spans, splats, capacity=cap)
    for r in (ref, got):
        assert int(r["tail"][-2]) == 1 and int(r["bins"].abs().max()) == 0
        assert bool((r["scattered"] == SENTINEL).all()) and bool((r["staged"] == SENTINEL).all())
        assert r["longest"] == UNSET
    assert torch.equal(ref["tail"], got["tail"])
    B.same(B.chain(inp, WALK, capacity=inp["total"]), _span_chain(inp, spans, splats, capacity=inp["total"]))


def _round(sigma):
    return [1.0 / sigma ** 2, 0.0, 1.0 / sigma ** 2]


def _six_and_seven_rows(rng):
    """round Gaussians centred in tile row 9: radius 40 -> rows 7..12 (six), radius 48 -> rows 6..12 (seven), alternating
    inside the first chunk; every seventh of them with the opacity of a logit of -12"""
    k = 600
    at = np.arange(k) * 2
    x = rng.uniform(60.0, W - 60.0, k)
    y = np.full(k, 152.0)
    rad = np.where(np.arange(k) % 2 == 0, 40, 48)
    con = np.array([_round(r / 3.0) for r in rad])
    op = np.where(np.arange(k) % 7 == 3, 1.0 / (1.0 + np.exp(12.0)), 0.8)
    return at, np.stack([x, y], 1), rad, con, op


def test_six_and_seven_rows_in_one_chunk(host):
    inp = _inputs("six and seven", craft=_six_and_seven_rows)
    st, ref, spans, _ = _check(host, inp)
    r = (spans[:1200:2, 0].cpu() >> 16) & 0xff
    culled = torch.arange(600) % 7 == 3
    assert bool((r[culled] == 0).all())                                       # TightTest::cull_all: nothing listed
    even, odd = r[(torch.arange(600) % 2 == 0) & ~culled], r[(torch.arange(600) % 2 == 1) & ~culled]
    assert bool((even == 6).all()) and bool((odd == 0xff).all())              # six rows held, seven fall back


def test_257_tile_columns(host):
    """4112 x 48: a range that ends at column 256 is held (hi = 256), one that reaches column 256 falls back"""
    st, ref, _, _ = _check(host, _inputs("257 columns", dims=(4112, 48)))
    assert ref["nt"] == 257 * 3 and st["widest"] == 256 and 0 < st["fallback"] < N // 50


def _needles(rng):
    """horizontal needles ~40 tiles long (sigma 107 x 2 px, radius 320) on 1920 x 64: runs of more than 32 lists that
    cross the groups of a 120-column frame"""
    k = 300
    at = np.arange(k) * 3
    xy = np.stack([rng.uniform(300.0, 1620.0, k), rng.uniform(4.0, 60.0, k)], 1)
    con = np.tile([1.0 / 107.0 ** 2, 0.0, 0.25], (k, 1))
    return at, xy, np.full(k, 320), con, np.full(k, 0.9)


def test_long_needles(host):
    inp = _inputs("needles", dims=(1920, 64), craft=_needles)
    st, ref, spans, _ = _check(host, inp)
    s = spans[:900:3].cpu()
    rows = (s[:, 0] >> 16) & 0xff
    assert bool((rows <= 4).all()) and bool((rows >= 1).all())
    lo, hi = s[:, 1] & 0xff, ((s[:, 1] >> 8) & 0xff) + 1                      # the first row of every needle
    width = torch.maximum(hi - lo, (((s[:, 1] >> 24) & 0xff) + 1) - ((s[:, 1] >> 16) & 0xff))
    assert int(width.max()) >= 36 and ref["nt"] == 480


def _walk_hand_made(dims, ids, first, rows):
    """records written by hand for the Gaussians `ids` (first row, then up to six (lo, hi) rows each; hi <= lo: an empty
    row), bounding-box slots for everything they list, depth = id, every other input zeroed -> the chain's results and
    the sorted ids the records spell out"""
    dev = torch.device(DEV)
    tbx = (dims[0] + 15) // 16
    spans = np.zeros((N, 4), np.uint32)
    nth = np.zeros(N, np.int32)
    tiles, owners = [], []
    for i, f, rr in zip(ids, first, rows):
        spans[i, 0] = f | (len(rr) << 16)
        for k, (lo, hi) in enumerate(rr):
            v = (lo | ((hi - 1) << 8)) if hi > lo else 1
            spans[i, 1 + k // 2] |= v << (16 * (k % 2))
            t = (f + k) * tbx + np.arange(lo, max(lo, hi))
            tiles.append(t)
            owners.append(np.full(len(t), i))
            nth[i] += len(t)
    tiles, owners = np.concatenate(tiles), np.concatenate(owners)
    inp = dict(n=N, xys=torch.zeros((N, 2), device=dev), radii=torch.zeros((N,), dtype=torch.int32, device=dev),
               depths=torch.arange(N, dtype=torch.float32, device=dev),
               cum=torch.from_numpy(np.cumsum(nth).astype(np.int32)).to(dev), total=int(nth.sum()), tile_rows=None, dims=dims)
    got = _span_chain(inp, torch.from_numpy(spans.view(np.int32)).to(dev), None)
    order = np.lexsort((owners, tiles))
    want_ids = owners[order]
    want_len = np.bincount(tiles, minlength=got["nt"])
    assert got["listed"] == len(want_ids) and int(got["tail"][-2]) == 0
    assert np.array_equal(got["lens"].numpy(), want_len)
    assert np.array_equal(got["ids"].numpy(), want_ids)                      # depth = id: a sorted list is ascending ids
    return got, nth


def test_hand_made_records_with_an_empty_middle_row():
    """the walk lists what a record says, an empty row between two others included (no convex ellipse leaves such a
    row, so these records are written by hand)"""
    rng = np.random.default_rng(3)
    k = 500
    ids = np.sort(rng.choice(N, k, replace=False))
    first = rng.integers(0, 17, k)
    lo = rng.integers(0, 20, (k, 2))
    hi = lo + rng.integers(1, 6, (k, 2))                                     # <= 25 columns
    rows = [[(int(lo[j, 0]), int(hi[j, 0])), (1, 1), (int(lo[j, 1]), int(hi[j, 1]))] for j in range(k)]
    _walk_hand_made((W, H), ids, first, rows)


def test_runs_beyond_the_staging_buffer():
    """1920 x 64 (120 columns: a row of lists crosses up to four group boundaries).  The first chunk lists full rows in all
    four tile rows - more staged runs AND more pairs than the staging buffer holds; the second lists one full row per
    Gaussian - pairs beyond the buffer, runs within it; the third a few short runs: staged, expanded, copied out"""
    cap = _lib.load().ts_bin_stage_capacity()
    per = B.chunks(N)[1]
    ids = np.concatenate([np.arange(per), per + np.arange(per), 2 * per + np.arange(0, per, 3)])
    rng = np.random.default_rng(5)
    first, rows = [], []
    for i in ids:
        c = i // per
        if c == 0:
            first.append(0); rows.append([(0, 120)] * 4)
        elif c == 1:
            first.append(int(rng.integers(0, 4))); rows.append([(0, 120)])
        else:
            lo = int(rng.integers(0, 100))
            first.append(int(rng.integers(0, 3))); rows.append([(lo, lo + int(rng.integers(1, 20))), (lo + 3, lo + 4)])
    got, nth = _walk_hand_made((1920, 64), ids, first, rows)
    pairs = [int(nth[c * per:(c + 1) * per].sum()) for c in range(3)]
    runs = [per * 4 * 4, per * 4, None]                                      # 120 columns from 0: four groups per row
    assert pairs[0] > cap and runs[0] > cap and pairs[1] > cap and runs[1] <= cap and 0 < pairs[2] <= cap


# ---- frames -----------------------------------------------------------------------------------------------------------
def _frames(model, cam, dims, depth, tight=True):
    """the frame with frame.ROW_SPANS off, on, on -> the results of each.  (No balanced-walk hint, whatever the frame in
    front listed per Gaussian: with it the executor takes the group form, which has no use for records)"""
    lib = _lib.load()
    saved = (frame.ROW_SPANS, frame.WIDE_TILES, frame.TIGHT_BINNING, frame.BALANCED_WALK_FROM)
    res, spans = [], None
    try:
        frame.WIDE_TILES, frame.TIGHT_BINNING, frame.BALANCED_WALK_FROM = 0, tight, float("inf")
        for on in (False, True, True):
            frame.ROW_SPANS = on
            out, F = _render(model, cam, dims, 1, depth)
            assert bool(F.fr.flags & _lib.FRAME_ROW_SPANS) == on and bool(F.fr.row_spans) == on
            assert bool(F.fr.flags & _lib.FRAME_ONE_WALK) and lib.ts_bin_one_walk_form(F.n, F.num_tiles) == 1
            assert not (F.fr.cam.hints & _lib.HINT_BALANCED_WALK)
            b = frame.last_binning[0]
            bins = b.tile_bins.clone()
            nws = int(lib.ts_bin_ws_ints(F.n, F.num_tiles))
            base = F.wf.data_ptr()
            tail = F.wf[F.fr.bin_ws - base:][:4 * nws].view(torch.int32)[-(F.num_tiles + 3):].clone()
            word = ctypes.c_int32.from_address(frame._pinned_total[0][0].data_ptr() + 4).value
            assert word == int((bins[:, 1] - bins[:, 0]).max()) > 0 and int(tail[-2]) == 0
            res.append(out + [bins, b.gaussian_ids_sorted[:int(bins[:, 1].max())].clone(), tail])
            if on:
                spans = F.wf[F.fr.row_spans - base:][:16 * F.n].view(torch.int32).view(-1, 4).cpu()
    finally:
        frame.ROW_SPANS, frame.WIDE_TILES, frame.TIGHT_BINNING, frame.BALANCED_WALK_FROM = saved
    assert len(res[0]) == (13 if depth else 12)        # image, final state[, depth], xys.grad, six parameters, lists, tail
    for a, b, c in zip(*res):
        assert a.shape == b.shape and torch.equal(a, b)       # walked from the records == computed by the walk
        assert torch.equal(b, c)                              # and repeats itself
    return res, (spans[:, 0] >> 16) & 0xff


@pytest.mark.parametrize("depth", [False, True])
def test_frame_bitwise(depth):
    model, cam = make_scene(N, 1, W, H, seed=43)
    res, rows = _frames(model, cam, (W, H), depth)
    assert float(res[0][0].max()) > 0.1
    assert int((rows > 0).sum()) > N // 2 and int(rows.max()) <= 6            # every record written, none falls back


def test_frame_bitwise_with_fallback_records_and_faint_gaussians():
    """a third of the Gaussians enlarged 2 to 24 times (boxes beyond six rows beside boxes of one) and every seventh
    opacity logit at -12, RGB + depth"""
    model, cam = make_scene(N, 1, W, H, seed=44)
    g = torch.Generator().manual_seed(9)
    k = N // 3
    with torch.no_grad():
        model.scales[:k] += torch.log(2.0 + 22.0 * torch.rand((k, 1), generator=g))
        model.opacities[::7] = -12.0
    res, rows = _frames(model, cam, (W, H), True)
    assert int((rows == 0xff).sum()) > 1000 and int((rows == 6).sum()) > 100


def test_frame_bitwise_bounding_box_lists():
    model, cam = make_scene(N, 1, W, H, seed=43)
    _frames(model, cam, (W, H), False, tight=False)


def test_frame_bitwise_257_tile_columns():
    model, cam = make_scene(N, 1, 4112, 48, seed=45)
    res, rows = _frames(model, cam, (4112, 48), False)
    assert int((rows == 0xff).sum()) > 0
