"""The pass boundaries of the fine hop (csrc/binning.hip) against a host expectation that needs no oracle.  The fine hop
streams the entries of a group of 32 lists in passes - 8 192 entries in the matrix and group forms, 20 480 in the one-walk
form - and a group of more than one pass is counted before it is placed.  Here the inputs are built directly: 2^18
Gaussians of radius 1, each centred in one tile of a 400 x 304 frame (475 tiles: 14 full groups and one of 27) and listed
without the tight test (splats = NULL), so every Gaussian lists exactly that tile, cum_tiles_hit is 1..n, tile_bins is a
bincount and a cumulative sum, and a list is its ids ordered by depth (a seeded permutation of n distinct values).  All
three two-hop forms run through the C ABI and are compared with that expectation bit for bit."""
import pytest
import torch

from binning_cases import DEV, GROUP, H, MATRIX, W, WALK, chain

pytestmark = pytest.mark.gpu
N = 1 << 18
TILES, GROUPS = 475, 15
# Entries per group, around the two pass sizes - kFinePass = 8 192 (bin_scatter_fine_kernel, bin_scatter_fine_groups_kernel)
# and kRunPass = 20 480 (bin_scatter_fine_runs_kernel), private constants of csrc/binning.hip: a change to either needs new
# populations here.  The three groups left over (the last one is the group of 27 lists) share the remaining 61 437.
POPULATIONS = [0, 1, 8191, 8192, 8193, 16384, 16385, 20479, 20480, 20481, 40960, 40961]
REST = N - sum(POPULATIONS)
POPULATIONS += [REST // 3, REST // 3, REST - 2 * (REST // 3)]
SORT_CAP = 4096             # kSortCap: ts_sort_tiles counts the lists beyond it in the spare word
_cases = {}


def _case(placement):
    """inputs of binning_cases.chain and the host expectation"""
    if placement not in _cases:
        assert REST == 61437 and len(POPULATIONS) == GROUPS and sum(POPULATIONS) == N
        gen = torch.Generator().manual_seed(7)
        tile = []
        for g, pop in enumerate(POPULATIONS):
            width = min(32, TILES - 32 * g)
            k = torch.arange(pop)
            # all entries of the group in one of its tiles (a different one from group to group), or dealt round its tiles
            tile.append(32 * g + ((k % width) if placement == "round robin" else torch.full((pop,), (5 * g) % width)))
        tile = torch.cat(tile)[torch.randperm(N, generator=gen)]          # the groups mixed through every chunk
        rank = torch.randperm(N, generator=gen)
        xys = torch.stack([16.0 * (tile % 25) + 8.0, 16.0 * (tile // 25) + 8.0], 1).float().contiguous()
        dev = torch.device(DEV)
        inp = dict(n=N, xys=xys.to(dev), depths=(rank + 1).float().to(dev),
                   radii=torch.ones(N, dtype=torch.int32, device=dev), splats=None,
                   cum=torch.arange(1, N + 1, dtype=torch.int32, device=dev), total=N, tile_rows=None, dims=(W, H))
        counts = torch.bincount(tile, minlength=TILES)
        end = counts.cumsum(0)
        start = end - counts
        bins = torch.where((counts > 0)[:, None], torch.stack([start, end], 1), torch.zeros(TILES, 2, dtype=torch.long))
        want = dict(bins=bins.int(), ids=torch.argsort(tile * N + rank).int(),
                    tail=torch.cat([start, torch.tensor([N, 0, int((counts > SORT_CAP).sum())])]).int(),
                    longest=int(counts.max()))
        _cases[placement] = (inp, want)
    return _cases[placement]


@pytest.mark.parametrize("form", [MATRIX, GROUP, WALK])
@pytest.mark.parametrize("placement", ["one tile", "round robin"])
def test_pass_boundaries(placement, form):
    inp, want = _case(placement)
    got = chain(inp, form)
    assert got["nt"] == TILES and got["listed"] == N
    assert torch.equal(got["bins"], want["bins"])
    assert torch.equal(got["ids"], want["ids"])
    assert torch.equal(got["tail"], want["tail"])               # tile_start[0..T], guard word, spare word
    assert got["longest"] == want["longest"]
