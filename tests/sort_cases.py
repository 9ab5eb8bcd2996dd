"""Inputs of the per-tile depth sort built on the host - no binning, no scene - and their host order.

The sort entries (ts_sort_tiles, ts_sort_tiles_stats, ts_sort_tiles_above, and the sort inside ts_raster_fwd_sort) read
only tile_bins, depths and bucket_ids.  Here every tile gets a list of a chosen LENGTH around the lengths at which the
sort changes its form, the number E of keys per lane, the padding or the run split; the ids of a list are a random subset,
without repeats, of one pool of Gaussians (sparse inside a list, shared between lists); the depths come from one of four
POPULATIONS and the bucket from one of four ORDERS.  The expectation of a tile is np.lexsort((id, depth bits)): the key
contract of make_key (csrc/sort_network.h) for non-negative floats.

numpy only: tests/test_sort_cases_cpu.py checks the conditions on these inputs without a GPU, tests/test_gpu_sort_forms.py
runs the kernels on them."""
import numpy as np

# ---- private constants of the kernels, restated: a change to any of them needs new lengths here ----------------------
WAVE_SORT_MAX = 1024    # kWaveSortMax (csrc/sort_network.h:130): one wave's register network, sort_tile_wave<E>, E = 1, 2,
#                         4, 8, 16 for n <= 64, 128, 256, 512, 1024 (csrc/binning.hip:1386-1390, csrc/raster.hip:1090-1094)
SORT_CAP = 4096         # kSortCap (csrc/binning.hip:1179): the workgroup network sort_tile_regs<E>, E = 1 .. 16 for
#                         n <= 256 E (sort_bucket_block, csrc/binning.hip:1243-1247); beyond: sort_tile_sample
WAVE_SUB_MAX = 256      # a sub-bucket of the sample sort up to this size is sorted by one wave (csrc/binning.hip:1333)
SAMPLE_WIDE = 8192      # n > 8192: 1024 samples instead of 256 (csrc/binning.hip:1279)
SUB_TARGET = 96         # kSubTarget (csrc/binning.hip:1265): nb = n / 96 sub-buckets ...
MAX_SUB = 512           # kMaxSub (csrc/binning.hip:1264): ... capped at 512, reached at n = 49 152
# cooperative tiles (coop_sort_tile<E>, csrc/raster.hip:803-813): n <= 128 wave 0 alone, then four runs of (n + 3) >> 2
# keys with E = 1, 2, 4 for n <= 256, 512, 1024

LENGTHS = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257,
           511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049,
           4095, 4096, 4097, 4352, 4500, 8191, 8192, 8193, 12000, 49151, 49152, 49153,
           200000]
POOL = 250_000                  # Gaussians: more than the longest list, fewer than the 417 370 entries of all lists
POPULATIONS = ["distinct", "four values", "all equal", "edge bits"]
ORDERS = ["random", "sorted", "reverse", "samples first"]
SEED = 12
SENTINEL = -1

_memo = {}


def sample_plan(n):
    """sort_tile_sample (csrc/binning.hip:1279-1281) -> (samples ns, shift of the sample positions, sub-buckets nb)"""
    ns, shift = (1024, 10) if n > SAMPLE_WIDE else (256, 8)
    return ns, shift, min(max(n // SUB_TARGET, 2), MAX_SUB)


def sample_positions(n):
    """positions (j * n) >> 8, or >> 10 for n > 8192, j = 0 .. ns - 1 (csrc/binning.hip:1287 and :1293)"""
    ns, shift, _ = sample_plan(n)
    return (np.arange(ns, dtype=np.int64) * n) >> shift


def sub_bucket_sizes(keys):
    """sizes of the sub-buckets sort_tile_sample cuts a bucket into; keys: uint64, in bucket order.  Splitter j
    (j = 0 .. nb - 2) = sorted sample[((j + 1) * ns) / nb], sub-bucket of a key = number of splitters <= key
    (sub_of, csrc/binning.hip:1302-1309)"""
    n = len(keys)
    ns, _, nb = sample_plan(n)
    smp = np.sort(keys[sample_positions(n)])
    splitters = smp[((np.arange(nb - 1, dtype=np.int64) + 1) * ns) // nb]
    return np.bincount(np.searchsorted(splitters, keys, side="right"), minlength=nb)


def make_keys(depths, ids):
    """make_key (csrc/sort_network.h:7): depth bits << 32 | id"""
    return (depths.view(np.uint32)[ids].astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)


def host_order(depths, ids):
    return ids[np.lexsort((ids, depths.view(np.uint32)[ids]))]


def depth_population(name, pool, rng):
    f32 = np.float32
    if name == "distinct":
        return (rng.permutation(pool) + 1).astype(f32) * f32(0.25)
    if name == "four values":                  # two of them one ulp apart: the order rests on the id
        vals = np.array([1.0, np.nextafter(f32(1.0), f32(2.0)), 2.5, 7.0], dtype=f32)
        return vals[rng.integers(0, 4, pool)]
    if name == "all equal":
        return np.full(pool, 3.0, dtype=f32)
    assert name == "edge bits"                 # non-negative floats only: the key contract
    d = (rng.permutation(pool) + 1).astype(f32) * f32(0.25)
    fi = np.finfo(f32)
    edges = np.array([0.0, fi.smallest_subnormal, np.nextafter(fi.tiny, f32(0.0)), fi.max, np.inf], dtype=f32)
    assert edges[2] < fi.tiny and (edges.view(np.uint32) >> 31 == 0).all()
    pick = rng.random(pool) < 0.3
    d[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    return d


def arrange(ids, depths, order, rng):
    """a list's ids in one bucket order"""
    n = len(ids)
    want = host_order(depths, ids)
    if order == "sorted":
        return want
    if order == "reverse":
        return want[::-1].copy()
    if order == "random" or n <= SORT_CAP:     # (no sample sort below: "samples first" is the random order there)
        return ids[rng.permutation(n)]
    assert order == "samples first"            # the ns sampled positions hold the ns smallest keys, in random order
    ns = sample_plan(n)[0]
    pos = sample_positions(n)
    assert len(np.unique(pos)) == ns
    out = np.empty(n, dtype=ids.dtype)
    out[pos] = want[:ns][rng.permutation(ns)]
    rest = np.ones(n, dtype=bool)
    rest[pos] = False
    out[rest] = want[ns:][rng.permutation(n - ns)]
    return out


def _lists(lengths, pool, seed, place):
    """tile of every length (a shuffled placement unless one is given) and the id subsets, shared by the populations and
    orders"""
    key = ("lists", tuple(lengths), pool, seed)
    if key not in _memo:
        rng = np.random.default_rng(seed)
        if place is None:
            place = rng.permutation(len(lengths))                   # tile t holds the list of length lengths[place[t]]
        _memo[key] = (place, [rng.choice(pool, lengths[k], replace=False).astype(np.int32) for k in place])
    return _memo[key]


def build(lengths, pool, population, order, seed, place=None):
    place, subsets = _lists(lengths, pool, seed, place)
    rng = np.random.default_rng([seed, POPULATIONS.index(population), ORDERS.index(order)])
    depths = depth_population(population, pool, np.random.default_rng([seed, POPULATIONS.index(population)]))
    lens = np.array([lengths[k] for k in place], dtype=np.int64)
    end = np.cumsum(lens)
    start = end - lens
    bins = np.where((lens > 0)[:, None], np.stack([start, end], 1), 0).astype(np.int32)   # empty tiles: (0, 0)
    bucket = np.concatenate([arrange(s, depths, order, rng) for s in subsets]).astype(np.int32)
    expect = np.concatenate([host_order(depths, s) for s in subsets]).astype(np.int32)
    return dict(tile_bins=bins, depths=depths, bucket_ids=bucket, expect=expect, lens=lens, listed=int(end[-1]),
                population=population, order=order)


def case(population, order):
    """the 38 lists of LENGTHS, one tile each"""
    key = ("case", population, order)
    if key not in _memo:
        _memo[key] = build(LENGTHS, POOL, population, order, SEED)
    return _memo[key]


def tile_slices(c):
    """(tile, length, slice of the list) of every non-empty tile"""
    return [(t, int(n), slice(int(b[0]), int(b[1]))) for t, (n, b) in enumerate(zip(c["lens"], c["tile_bins"])) if n > 0]


# ---- the frame of the sorts inside the forward compositing launch ----------------------------------------------------
# in-kernel lengths: those of up to 1025 entries, plus 2049 and 4097 (which ts_sort_tiles_above sorts before the launch),
# each twice on an 8 x 6 tile frame that is no multiple of 16 in either direction
FRAME_LENGTHS = [n for n in LENGTHS if n <= 1025] + [2049, 4097]
FRAME_W, FRAME_H = 123, 89
FRAME_TBX, FRAME_TBY = 8, 6
FRAME_TILES = FRAME_TBX * FRAME_TBY
FRAME_POOL = 6000               # more than 4097, fewer than the 24 400 entries of the frame
FRAME_POPULATIONS = ["distinct", "four values", "edge bits"]
FRAME_COOP16 = 8                # TS_CAM_COOP_TILES(8): half of every band cooperative


def coop_tiles(num_tiles, c16):
    """fwd_plan of csrc/raster.hip (:622-645, no list segments) -> mask of the tiles composited by a cooperative
    workgroup: a band is 4 * ceil(ceil(T / 4) / 8) tiles (one per XCD), and the first floor(per_xcd * C16 / 16) groups of
    four tiles of every band are cooperative (csrc/raster.hip:1027-1031)"""
    per_xcd = ((num_tiles + 3) // 4 + 7) // 8
    band = 4 * per_xcd
    coop = (per_xcd * c16) // 16
    return (np.arange(num_tiles) % band) < 4 * coop


def frame_place():
    """tile -> index into FRAME_LENGTHS: every length once on the tiles that TS_CAM_COOP_TILES(8) makes cooperative and once
    on the others, both in shuffled order"""
    assert 2 * len(FRAME_LENGTHS) == FRAME_TILES
    coop = coop_tiles(FRAME_TILES, FRAME_COOP16)
    rng = np.random.default_rng(SEED + 1)
    place = np.empty(FRAME_TILES, dtype=np.int64)
    place[coop] = rng.permutation(len(FRAME_LENGTHS))
    place[~coop] = rng.permutation(len(FRAME_LENGTHS))
    return place


def frame_case(population):
    """the lists of the frame (random bucket order) and the Gaussians behind them: distinct colours, and so wide that
    alpha is the opacity (to within 1 %) all over the frame.  Opacities of 0.005 .. 0.008: a list of 1024 entries leaves
    a transmittance of at least 0.992^1024 = 2.7e-4 > 1e-4, so every list of up to 1024 entries is walked to its end"""
    key = ("frame", population)
    if key not in _memo:
        # (the same length twice needs two subsets: the lengths are listed twice and placed by index)
        lengths = FRAME_LENGTHS + FRAME_LENGTHS
        coop = coop_tiles(FRAME_TILES, FRAME_COOP16)
        place = frame_place() + np.where(coop, 0, len(FRAME_LENGTHS))
        c = build(lengths, FRAME_POOL, population, "random", SEED + 2, place=place)
        rng = np.random.default_rng(SEED + 3)
        n = FRAME_POOL
        f32 = np.float32
        c["xys"] = (np.array([FRAME_W / 2, FRAME_H / 2]) + rng.uniform(-3.0, 3.0, (n, 2))).astype(f32)
        c["conics"] = np.tile(np.array([1e-7, 0.0, 1e-7], dtype=f32), (n, 1))
        c["radii"] = np.full(n, 4096, dtype=np.int32)             # the tile box of every Gaussian is the whole frame
        c["cum"] = ((np.arange(n) + 1) * FRAME_TILES).astype(np.int32)
        c["colors"] = rng.uniform(0.05, 1.0, (n, 4)).astype(f32)
        c["opacity"] = rng.uniform(0.005, 0.008, n).astype(f32)
        c["coop"] = coop
        _memo[key] = c
    return _memo[key]
