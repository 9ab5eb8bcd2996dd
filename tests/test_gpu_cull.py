"""The two alpha culls as the KERNELS run them, on hand-built 2-D inputs through the C ABI (no 3-D scene):
ts::TightTest inside ts_bin_count / ts_bin_scatter (device log2, walk_chunk, wide lists, tile-row stripes) and
ts::rect_may_contribute inside the compositing kernels (stage_splat, and the survivor lists raster_bwd replays).

Reference: alpha in float64 at every sample of a tile (tests/cull_cases.py) from the records READ BACK from the device,
and the float64 oracle image.  tests/test_hostmath_cull.py holds the same header, compiled for the host, to the same
contract on many more cases; this file binds the device code to it.
"""
import ctypes

import numpy as np
import pytest
import torch

import cull_cases as C
from oracle import gsplat_oracle as O
from tinysplat_amd import _lib, ops
from tinysplat_amd.rasterizer import tile_bounds

from test_gpu_parity import _raster_parity, _to_dev
from test_hostmath_cull import _tile_keep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = 640, 400
N_PER_FAMILY = 300
STRIPE = (7, 15)


def _inputs():
    recs, radii = [], []
    for k, family in enumerate(C.TILE_FAMILIES):
        r, rad = C.tile_cases(family, 6000 + k, N_PER_FAMILY, W, H)
        recs.append(r); radii.append(rad)
    return np.concatenate(recs), np.concatenate(radii)


def _box_counts(recs, radii, w, h, tile_rows):
    """num_tiles_hit as the projection kernel would write it: the tiles of ts::tile_bbox inside the stripe"""
    tb = tile_bounds((w, h))
    minx, miny, maxx, maxy = O.tile_bbox(torch.from_numpy(recs[:, :2].copy()), torch.from_numpy(radii).float(), tb)
    r0, r1 = (0, tb[1]) if tile_rows is None else tile_rows
    miny, maxy = miny.clamp(min=r0), maxy.clamp(max=r1)
    return ((maxx - minx).clamp(min=0) * (maxy - miny).clamp(min=0)).to(torch.int32)


def _lists(recs, radii, w, h, tight, wide=False, tile_rows=None):
    """ts_scan_tiles -> ts_pack_splats -> ts_bin_count / ts_tile_offsets / ts_bin_scatter -> ts_sort_tiles.
    -> (gaussian, list index) of every listed pair as a sorted int64 key array, the number of lists per row, the records
    read back [n, 6], the camera"""
    lib = _lib.load()
    dev = torch.device(DEV)
    n = len(recs)
    tb = tile_bounds((w, h))
    cam = ops._camera(0.0, 0.0, 0.0, 0.0, h, w, tb, tile_rows=tile_rows, wide_tiles=wide)
    nth = _box_counts(recs, radii, w, h, tile_rows).to(dev)
    t = torch.from_numpy(recs).to(dev)
    xys, opac, conics = t[:, :2].contiguous(), t[:, 2:3].contiguous(), t[:, 3:6].contiguous()
    rad = torch.from_numpy(radii).to(dev)
    g = torch.Generator().manual_seed(1)
    depths = torch.rand(n, generator=g).to(dev)
    colors = torch.rand(n, 3, generator=g).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    s = ops._stream(dev)
    p = ops._ptr
    nt = int(lib.ts_num_tiles(ctypes.byref(cam)))
    cum = torch.empty((n,), **i32)
    ws = torch.empty((int(lib.ts_scan_ws_ints(n)),), **i32)
    ops._call("ts_scan_tiles", lib.ts_scan_tiles, n, p(nth), p(cum), p(ws), None, s)
    total = int(cum[-1])
    assert total == int(nth.sum())
    splats = torch.zeros((n, 12), dtype=torch.float32, device=dev)
    ops._call("ts_pack_splats", lib.ts_pack_splats, n, 3, 0, p(xys), p(rad), p(conics), p(colors), p(opac), p(cum), cam,
              None, p(splats), s)
    bin_ws = torch.empty((int(lib.ts_bin_ws_ints(n, nt)),), **i32)
    tile_bins = torch.empty((nt, 2), **i32)
    tl = p(splats) if tight else None
    ops._call("ts_bin_count", lib.ts_bin_count, n, p(xys), p(rad), tl, cam, p(bin_ws), s)
    ops._call("ts_tile_offsets", lib.ts_tile_offsets, n, nt, p(bin_ws), p(tile_bins), None, -1, s)
    bins = tile_bins.cpu().numpy().astype(np.int64)
    listed = int(bins[:, 1].max())
    # the buffers below hold `total` entries: the lists must fit BEFORE anything is scattered into them
    assert 0 <= listed <= total and (bins[:, 0] <= bins[:, 1]).all() and bins.min() >= 0
    if not tight and not wide:
        assert listed == total
    bucket_ids = torch.full((max(total, 1),), -1, **i32)
    ids = torch.full((max(total, 1),), -1, **i32)
    ops._call("ts_bin_scatter", lib.ts_bin_scatter, n, p(xys), p(rad), tl, cam, p(bin_ws), p(bucket_ids), p(ids), s)
    ops._call("ts_sort_tiles", lib.ts_sort_tiles, nt, p(tile_bins), p(depths), p(bucket_ids), p(ids), p(bin_ws),
              bin_ws.data_ptr() + 4 * (bin_ws.numel() - 1), s)
    torch.cuda.synchronize()
    ids = ids.cpu().numpy().astype(np.int64)
    lens = bins[:, 1] - bins[:, 0]
    assert lens.sum() == listed
    entry_list = np.empty(listed, dtype=np.int64)
    for li in range(nt):
        entry_list[bins[li, 0]:bins[li, 1]] = li
    gid = ids[:listed]
    assert ((gid >= 0) & (gid < n)).all()
    # depth order inside every list
    d = depths.cpu().numpy()[gid]
    same = entry_list[1:] == entry_list[:-1]
    assert (d[1:][same] >= d[:-1][same]).all()
    keys = np.sort(gid * nt + entry_list)
    assert (np.diff(keys) > 0).all(), "a pair is listed twice"
    return keys, nt, splats[:, :6].cpu().numpy(), cam


_cache = {}


def _reference():
    """bounding-box lists of the device (splats NULL), and `needed` per bounding-box pair in float64 from the records
    the device packed"""
    if "ref" not in _cache:
        recs, radii = _inputs()
        box_keys, nt, back, cam = _lists(recs, radii, W, H, tight=False)
        tbx = cam.tile_bounds_x
        gi, t = box_keys // nt, box_keys % nt
        tx, ty = t % tbx, t // tbx
        # the record of every listed Gaussian is, bit for bit, what went in
        listed = np.unique(gi)
        assert np.array_equal(back[listed].view(np.uint32), recs[listed].view(np.uint32))
        amax = C.tile_alpha_max(back, gi, tx, ty)
        _cache["ref"] = (recs, radii, box_keys, nt, tbx, gi, tx, ty, amax >= C.ALPHA_MIN)
    return _cache["ref"]


def test_bounding_box_lists_are_the_boxes(hostmath):
    recs, radii, box_keys, nt, tbx, gi, tx, ty, needed = _reference()
    _, (g2, x2, y2), _ = _tile_keep(hostmath, recs, radii, W, H)
    assert np.array_equal(box_keys, np.sort(g2 * nt + y2 * tbx + x2))
    assert needed.any() and (~needed).any()


def test_tight_lists_hold_every_needed_pair_and_only_box_pairs(hostmath):
    recs, radii, box_keys, nt, tbx, gi, tx, ty, needed = _reference()
    keys, nt2, back, _ = _lists(recs, radii, W, H, tight=True)
    assert nt2 == nt
    assert np.isin(keys, box_keys, assume_unique=True).all(), "a tight pair outside the bounding box"
    kept = np.isin(box_keys, keys, assume_unique=True)
    bad = np.nonzero(needed & ~kept)[0]
    # (the device takes log2 from the hardware, the host from libm: their kept sets may differ; counted, not asserted)
    _, (g2, x2, y2), hk = _tile_keep(hostmath, recs, radii, W, H)
    host_set = np.sort((g2 * nt + y2 * tbx + x2)[hk])
    disagree = len(np.setxor1d(host_set, keys, assume_unique=True))
    print(f"[cull] device tight lists: bounding-box pairs {len(box_keys)}, needed {int(needed.sum())}, kept {len(keys)}, "
          f"kept/needed {len(keys) / max(int(needed.sum()), 1):.3f}, share of the box pairs {len(keys) / len(box_keys):.4f}, "
          f"pairs the host build of the header decides differently {disagree}")
    assert len(bad) == 0, (f"{len(bad)} needed pairs are missing from the tight lists; first: Gaussian {gi[bad[0]]} "
                           f"record {back[gi[bad[0]]].tolist()} radius {radii[gi[bad[0]]]} tile ({tx[bad[0]]}, {ty[bad[0]]})")
    assert len(keys) < len(box_keys)                         # and the lists are tight


def test_tight_wide_lists_hold_every_needed_pair():
    """wide_tiles = 1: a list is two horizontally adjacent 16x16 tiles"""
    recs, radii, box_keys, nt, tbx, gi, tx, ty, needed = _reference()
    wide_box, ntw, _, cam = _lists(recs, radii, W, H, tight=False, wide=True)
    keys, _, _, _ = _lists(recs, radii, W, H, tight=True, wide=True)
    tbw = (tbx + 1) // 2
    assert ntw == tbw * cam.tile_rows
    as_wide = lambda m: np.unique(gi[m] * ntw + ty[m] * tbw + (tx[m] >> 1))
    assert np.array_equal(wide_box, as_wide(np.ones(len(gi), dtype=bool)))
    assert np.isin(keys, wide_box, assume_unique=True).all()
    need_w = as_wide(needed)
    print(f"[cull] device tight wide lists: box pairs {len(wide_box)}, needed {len(need_w)}, kept {len(keys)}")
    assert np.isin(need_w, keys, assume_unique=True).all()
    assert len(keys) < len(wide_box)


def test_tight_lists_of_a_tile_row_stripe_hold_every_needed_pair():
    """tile_row0 > 0: list index = (ty - tile_row0) * tile_bounds_x + tx"""
    recs, radii, box_keys, nt, tbx, gi, tx, ty, needed = _reference()
    r0, r1 = STRIPE
    nts = (r1 - r0) * tbx
    m = (ty >= r0) & (ty < r1)
    as_stripe = lambda sel: np.sort(gi[sel] * nts + (ty[sel] - r0) * tbx + tx[sel])
    box_s, nt2, _, _ = _lists(recs, radii, W, H, tight=False, tile_rows=STRIPE)
    assert nt2 == nts
    assert np.array_equal(box_s, as_stripe(m))
    keys, _, _, _ = _lists(recs, radii, W, H, tight=True, tile_rows=STRIPE)
    assert np.isin(keys, box_s, assume_unique=True).all()
    need_s = as_stripe(m & needed)
    print(f"[cull] device tight stripe lists rows {r0}..{r1}: box pairs {len(box_s)}, needed {len(need_s)}, kept {len(keys)}")
    assert np.isin(need_s, keys, assume_unique=True).all()
    assert len(keys) < len(box_s)
    # the stripe's decisions are those of the full frame
    full, _, _, _ = _lists(recs, radii, W, H, tight=True)
    fg, ft = full // nt, full % nt
    fm = (ft // tbx >= r0) & (ft // tbx < r1)
    assert np.array_equal(keys, np.sort(fg[fm] * nts + (ft[fm] - r0 * tbx)))


# ---------------------------------------------------------------------------------------------------------------------
# the block cull inside compositing
# ---------------------------------------------------------------------------------------------------------------------
def _composite_args():
    xys, depths, radii, conics, colors, opac, bg = (torch.from_numpy(a) for a in C.composite_inputs())
    w, h = C.COMPOSITE_W, C.COMPOSITE_H
    minx, miny, maxx, maxy = O.tile_bbox(xys, radii.float(), tile_bounds((w, h)))
    nth = ((maxx - minx) * (maxy - miny)).to(torch.int32)
    radii = torch.where(nth > 0, radii, torch.zeros_like(radii))
    return [xys, depths, radii, conics, nth, colors, opac, h, w, bg], h, w


def test_block_cull_inside_compositing_against_the_float64_oracle():
    """cull_cases.composite_inputs: every Gaussian has one 8x8 block decided near its level set, colour minus
    background is ~1 and the lists are the bounding-box lists, so a block rejected although it is needed shows as an
    error of up to 1/255 = 4e-3 where 1e-5 is asserted; the gradients go through the survivor lists of the forward."""
    args, h, w = _composite_args()
    _raster_parity(args, h, w)


def test_compositing_is_bitwise_repeatable():
    args, h, w = _composite_args()
    g = torch.Generator().manual_seed(3)
    w_img, w_a = torch.rand(h, w, 3, generator=g).to(DEV), torch.rand(h, w, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        ops.clear_binning_cache()
        da = _to_dev(args)
        leaves = {i: da[i].clone().requires_grad_(True) for i in (0, 3, 5, 6)}
        for i, t in leaves.items():
            da[i] = t
        img, alpha = ops.rasterize_gaussians(*da)
        ((img * w_img).sum() + (alpha * w_a).sum()).backward()
        runs.append([img.detach(), alpha.detach()] + [leaves[i].grad for i in (0, 3, 5, 6)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][1].max() > 0.5
