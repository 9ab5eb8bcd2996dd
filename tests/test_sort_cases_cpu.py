"""Conditions on the inputs of tests/sort_cases.py, checked without the kernels: the expectation is a strict order of the
bucket, and a numpy restatement of the sample sort's splitter arithmetic and of the forward launch's plan shows WHICH form
of the sort every list reaches - so that tests/test_gpu_sort_forms.py cannot pass with a form never run."""
import numpy as np
import pytest

import sort_cases as S

CASES = [(p, o) for p in S.POPULATIONS for o in S.ORDERS]


def _sizes(c):
    """length -> sub-bucket sizes, for the lists of the sample sort"""
    return {n: S.sub_bucket_sizes(S.make_keys(c["depths"], c["bucket_ids"][sl])) for _, n, sl in S.tile_slices(c)
            if n > S.SORT_CAP}


def _show(population, order, sizes):
    """sub-buckets per path: one wave | workgroup network in place, E = 2, 4, 8, 16 | global-memory network"""
    edges = [0, 256, 512, 1024, 2048, S.SORT_CAP, 1 << 30]
    for n, sz in sorted(sizes.items()):
        print(f"{population} / {order}: n {n} largest {sz.max()} per path "
              f"{[int(((sz > lo) & (sz <= hi)).sum()) for lo, hi in zip(edges, edges[1:])]}")


def test_the_lengths_sit_on_every_boundary():
    assert len(S.LENGTHS) == len(set(S.LENGTHS)) == 38
    for edge in (64, 128, 256, 512, S.WAVE_SORT_MAX, 2048, S.SORT_CAP, S.SAMPLE_WIDE, S.SUB_TARGET * S.MAX_SUB):
        assert {edge - 1, edge, edge + 1} <= set(S.LENGTHS)
    assert max(S.LENGTHS) < S.POOL < sum(S.LENGTHS) < 500_000
    assert S.sample_plan(S.SUB_TARGET * S.MAX_SUB - 1)[2] == S.MAX_SUB - 1 and S.sample_plan(49152)[2] == S.MAX_SUB
    assert S.sample_plan(8192)[:2] == (256, 8) and S.sample_plan(8193)[:2] == (1024, 10)


@pytest.mark.parametrize("population,order", CASES)
def test_expectation_is_a_strict_order_of_the_bucket(population, order):
    c = S.case(population, order)
    assert c["listed"] == sum(S.LENGTHS) == len(c["bucket_ids"]) == len(c["expect"])
    assert sorted(c["lens"].tolist()) == sorted(S.LENGTHS)
    assert c["lens"].tolist() != sorted(S.LENGTHS)                       # mixed lengths per workgroup of four tiles
    assert (c["depths"].view(np.uint32) >> 31 == 0).all() and not np.isnan(c["depths"]).any()
    for t, n, sl in S.tile_slices(c):
        got, src = c["expect"][sl], c["bucket_ids"][sl]
        assert np.array_equal(np.sort(got), np.sort(src)) and len(np.unique(src)) == n
        keys = S.make_keys(c["depths"], got)
        assert (keys[1:] > keys[:-1]).all()
        if order == "random" and n >= 65:
            assert not np.array_equal(got, src)
    empty = c["lens"] == 0
    assert empty.sum() == 1 and (c["tile_bins"][empty] == 0).all()
    # ids are sparse inside a list and shared between lists
    assert len(np.unique(c["bucket_ids"])) < c["listed"] and c["bucket_ids"].max() >= max(S.LENGTHS)
    if population == "four values":
        assert len(np.unique(c["depths"])) == 4 and np.diff(np.sort(np.unique(c["depths"]).view(np.uint32)))[0] == 1
    if population == "edge bits":
        bits = set(np.unique(c["depths"].view(np.uint32)).tolist())
        assert {0x00000000, 0x00000001, 0x007FFFFF, 0x7F7FFFFF, 0x7F800000} <= bits


@pytest.mark.parametrize("population", S.POPULATIONS)
def test_sub_bucket_classes_of_the_random_order(population):
    """A sub-bucket spans ns / nb sample gaps of n / ns keys each.  Where that is six gaps or more (4097 .. 4500: 256
    samples for 42 .. 46 sub-buckets; 8193, 12000: 1024 for 85, 125) every sub-bucket stays within one wave's 256 keys.
    At 8191 / 8192 (three gaps of 32 keys) and from 49151 on (two gaps of 48) the size is a sum of two or three
    exponential gaps with a mean of 96, which exceeds 256 in 1 - 3 % of the sub-buckets whatever the seed (measured here:
    0 - 2 of 85, 9 - 20 of 512): those lists reach the in-place workgroup network as well, never the global one."""
    sizes = _sizes(S.case(population, "random"))
    _show(population, "random", sizes)
    assert sorted(sizes) == [n for n in S.LENGTHS if n > S.SORT_CAP]
    for n in (4097, 4352, 4500, 8193, 12000):
        assert sizes[n].max() <= S.WAVE_SUB_MAX, n
    for n, sz in sizes.items():
        assert sz.sum() == n and sz.max() <= S.SORT_CAP, n
        assert (sz <= S.WAVE_SUB_MAX).any()
    # the 200 000 list: sub-buckets in each of the E = 2, 4, 8 ranges of sort_bucket_block
    big = sizes[200000]
    for lo in (256, 512, 1024):
        assert ((big > lo) & (big <= 2 * lo)).any(), lo


@pytest.mark.parametrize("population", S.POPULATIONS)
def test_sub_bucket_classes_of_the_adversarial_order(population):
    """samples first: every unsampled key lies above every splitter and lands in the LAST sub-bucket"""
    sizes = _sizes(S.case(population, "samples first"))
    _show(population, "samples first", sizes)
    for n, sz in sizes.items():
        ns, _, nb = S.sample_plan(n)
        last = n - ((nb - 1) * ns) // nb                    # the samples from the last splitter on, and all the rest
        assert sz[-1] == last == sz.max() and (sz[:-1] <= S.WAVE_SUB_MAX).all(), n
    # 4097: the in-place workgroup network with E = 16; everything longer: the global-memory network
    assert 2048 < sizes[4097][-1] <= S.SORT_CAP
    assert sizes[4097][-1] == 3848 and sizes[4352][-1] == 4102          # (4352 lies six keys beyond the cap)
    for n in (4352, 4500, 8193, 12000, 49152, 200000):
        assert sizes[n][-1] > S.SORT_CAP, n
    assert (sizes[4500][-1], sizes[8193][-1], sizes[12000][-1]) == (4250, 7182, 10985)


@pytest.mark.parametrize("population", S.POPULATIONS)
@pytest.mark.parametrize("order", ["sorted", "reverse"])
def test_sub_bucket_classes_of_the_monotone_orders(population, order):
    sizes = _sizes(S.case(population, order))
    for n, sz in sizes.items():
        assert sz.max() <= (S.WAVE_SUB_MAX if n < 200000 else 1024), n


def test_cooperative_band_layout():
    """fwd_plan restated: with TS_CAM_COOP_TILES(8) on 48 tiles a band is 8 tiles and its first group of four is
    cooperative; the layout puts every in-kernel length once on a cooperative tile and once in a whole-tile wave"""
    coop = S.coop_tiles(S.FRAME_TILES, S.FRAME_COOP16)
    assert coop.tolist() == [t % 8 < 4 for t in range(48)]
    assert S.coop_tiles(48, 0).sum() == 0 and S.coop_tiles(48, 15).sum() == 24          # floor(2 * 15 / 16) = 1 group
    assert S.coop_tiles(8160, 8).sum() == 8 * 4 * 127                                   # 255 groups per band: floor(127.5)
    assert S.FRAME_W % 16 and S.FRAME_H % 16
    assert (S.FRAME_W + 15) // 16 == S.FRAME_TBX and (S.FRAME_H + 15) // 16 == S.FRAME_TBY
    want = [n for n in S.LENGTHS if n <= 1025] + [2049, 4097]
    for population in S.FRAME_POPULATIONS:
        c = S.frame_case(population)
        assert sorted(c["lens"][coop].tolist()) == sorted(c["lens"][~coop].tolist()) == want
        assert c["lens"][coop].tolist() != c["lens"][~coop].tolist()
        assert max(want) < S.FRAME_POOL < c["listed"] == 2 * sum(want)
        for t, n, sl in S.tile_slices(c):
            keys = S.make_keys(c["depths"], c["expect"][sl])
            assert (keys[1:] > keys[:-1]).all()
            assert np.array_equal(np.sort(c["expect"][sl]), np.sort(c["bucket_ids"][sl]))
            if n >= 65:
                assert not np.array_equal(c["expect"][sl], c["bucket_ids"][sl])
        # a list of up to 1024 entries never stops: the transmittance stays above kTEps = 1e-4
        op = c["opacity"].astype(np.float64)
        assert 0.005 <= op.min() and op.max() <= 0.008 and op.min() > 1.02 / 255
        for t, n, sl in S.tile_slices(c):
            if n <= S.WAVE_SORT_MAX:
                assert np.prod(1.0 - op[c["expect"][sl]]) > 2e-4
        assert len(np.unique(c["colors"], axis=0)) == S.FRAME_POOL
